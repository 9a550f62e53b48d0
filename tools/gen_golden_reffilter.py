#!/usr/bin/env python3
"""Generate tests/golden/reference_filter.npz from the thesis' recorded reference-filter output.

    python3 -B tools/gen_golden_reffilter.py <reference>/results/all_plots

Reads results/all_plots/{box_test,current_box_test,large_setpoints}/bagfile__{RL,QP}_reference_filter_state_desired.csv of the
reference (the ROS topic reference_filter/state_desired the RL node took its reference from, rl_allocator.py:160,187-195; about 10 Hz)
and fits the linear third-order reference model of include/dpenv.h to it, per axis N, E, psi:
    x''' + (2 zeta + 1) omega x'' + (2 zeta + 1) omega^2 x' + omega^3 x = omega^3 r
The position is a sum of unit step responses, one per setpoint switch: x_j(t) = r0_j + sum_k (r_k,j - r_k-1,j) s_j(t - t_k).
Two least-squares fits on position (N, E in m, heading in rad scaled by 5 m / (pi / 4)):
  * pinned: omega and zeta held at the library defaults (deploy.REFERENCE_FILTER_OMEGA / _ZETA); free: the switch times t_k and
    the targets r_k.  These targets and switch times are what tests/test_reference_filter_cpu.py replays.
  * free: omega_j and zeta_j free as well - the fit the defaults come from, kept for the record and printed.
Only data is written: the recorded samples (time from the start of the recording, position / velocity / acceleration made relative
to the first sample's position, heading in rad) and the fitted numbers.  Needs scipy (build side only)."""
import os
import sys

import numpy as np
from scipy.linalg import expm
from scipy.optimize import least_squares

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ml4ca_amd.deploy import REFERENCE_FILTER_OMEGA, REFERENCE_FILTER_ZETA   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'reference_filter.npz')
DIRS = ('box_test', 'current_box_test', 'large_setpoints')
RUNS = ('RL', 'QP')
W_PSI = 5.0 / (np.pi / 4)


def step_response(omega, zeta, tau):
    """Unit step response from rest of the reference model at times tau (0 for tau <= 0), exact (4x4 matrix exponential)."""
    c = 2.0 * zeta + 1.0
    M = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [-omega ** 3, -c * omega ** 2, -c * omega, omega ** 3], [0, 0, 0, 0]], np.float64)
    tp = np.maximum(tau, 0.0)
    E = expm(M[None] * tp[:, None, None])
    return np.where(tau > 0, E[:, 0, 3], 0.0)


def load(path):
    d = np.genfromtxt(path, delimiter=',')[1:]
    t = d[:, 10] - d[0, 10]
    pos = np.stack([d[:, 1] - d[0, 1], d[:, 2] - d[0, 2], np.deg2rad(d[:, 3])])
    vel = np.stack([d[:, 4], d[:, 5], np.deg2rad(d[:, 6])])
    acc = np.stack([d[:, 7], d[:, 8], np.deg2rad(d[:, 9])])
    return t, pos, vel, acc


def detect(t, pos, vel):
    """Initial guesses: a switch where the filter starts to move after resting; targets = where each segment settles."""
    moving = (np.abs(vel[0]) > 1e-3) | (np.abs(vel[1]) > 1e-3) | (np.abs(vel[2]) > 1e-4)
    starts = [i for i in range(1, len(t)) if moving[i] and not moving[max(i - 5, 0):i].any()]
    ends = starts[1:] + [len(t)]
    targets = [pos[:, 0]] + [pos[:, e - 1] for e in ends]
    return np.array([t[i - 1] for i in starts]), np.array(targets)


def model(t, r, ts, omega, zeta):
    x = np.repeat(r[0][:, None], len(t), 1)
    for k, tk in enumerate(ts):
        for j in range(3):
            dr = r[k + 1, j] - r[k, j]
            if dr != 0.0:
                x[j] += dr * step_response(omega[j], zeta[j], t - tk)
    return x


def fit(t, pos, ts0, r0, free):
    K = len(ts0)

    def unpack(p):
        ts, r = p[:K], p[K:K + 3 * (K + 1)].reshape(K + 1, 3)
        if free:
            om, ze = p[K + 3 * (K + 1):K + 3 * (K + 1) + 3], p[K + 3 * (K + 1) + 3:]
        else:
            om, ze = np.asarray(REFERENCE_FILTER_OMEGA), np.asarray(REFERENCE_FILTER_ZETA)
        return ts, r, om, ze

    def res(p):
        ts, r, om, ze = unpack(p)
        e = model(t, r, ts, om, ze) - pos
        e[2] *= W_PSI
        return e.ravel()

    p0 = np.concatenate([ts0, r0.ravel()] + ([np.asarray(REFERENCE_FILTER_OMEGA), np.asarray(REFERENCE_FILTER_ZETA)] if free else []))
    sol = least_squares(res, p0, x_scale='jac')
    ts, r, om, ze = unpack(sol.x)
    e = model(t, r, ts, om, ze) - pos
    return ts, r, om, ze, e


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    base = sys.argv[1]
    out = {}
    for d in DIRS:
        for run in RUNS:
            path = os.path.join(base, d, 'bagfile__%s_reference_filter_state_desired.csv' % run)
            t, pos, vel, acc = load(path)
            ts0, r0 = detect(t, pos, vel)
            ts, r, _, _, e = fit(t, pos, ts0, r0, free=False)
            tsf, rf, om, ze, ef = fit(t, pos, ts, r, free=True)
            key = '%s.%s' % (d, run)
            f32 = lambda x: x.astype(np.float32)                          # relative to the start: f32 keeps well below a micrometre
            out.update({key + '.t': f32(t), key + '.pos': f32(pos), key + '.vel': f32(vel), key + '.acc': f32(acc), key + '.switch_t': ts,
                        key + '.targets': r, key + '.free_omega': om, key + '.free_zeta': ze})
            print('%-28s %d switches  pinned: max |e| N/E %.4f m, psi %.3f deg (rms %.4f m)   free: omega %s zeta %s, max |e| %.4f m, %.3f deg'
                  % (key, len(ts), np.abs(e[:2]).max(), np.rad2deg(np.abs(e[2]).max()), np.sqrt((e[:2] ** 2).mean()),
                     np.round(om, 4), np.round(ze, 4), np.abs(ef[:2]).max(), np.rad2deg(np.abs(ef[2]).max())))
    out['default_omega'] = np.asarray(REFERENCE_FILTER_OMEGA)
    out['default_zeta'] = np.asarray(REFERENCE_FILTER_ZETA)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
