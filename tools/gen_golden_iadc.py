#!/usr/bin/env python3
"""Generate tests/golden/iadc.npz by running the reference's own box-test actuator script.

Runs ONLY in the build container (needs /root/reference); start as ``python3 -B tools/gen_golden_iadc.py``.

Executed as it is, with runpy, cwd in its directory (it opens its CSV files by bare name), behind a stub for matplotlib (absent here; the
IADC section never touches a figure):  results/all_plots/box_test/plot_act.py  ->  the IADC section (:320-391), its `derivs` (six
per-interval lists per contender: n_bow, a_bow = 0, n_port, a_port, n_star, a_star, each already multiplied by dt), `IADC` (the clipped
per-interval sums behind a leading 0) and `IADC_cumsums` (the running sums WITHOUT the last interval: cumsums[:-1]).
Input data: the recorded Cybersea box test, box_test/bagfile__{QP,RL}_{thrusterAllocation_stern_thruster_setpoints,
thrusterAllocation_pod_angle_input,bow_control}.csv as the script slices them (:48-60).  QP is the recording with intervals under 0.1 s
(the script's short-interval rule, :336-339 and :358-363, fires on it); RL has a regular grid of about 0.2 s.
Only data is written: the command and time series (inputs) and the script's three results (expected outputs), plus the totals the script
prints for all four contenders."""
import os
import runpy
import sys
from unittest import mock

sys.dont_write_bytecode = True
import numpy as np

REF = '/root/reference/results/all_plots/box_test'
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'iadc.npz')


def subplots(r=1, c=1, *args, **kw):
    axes = [mock.MagicMock() for _ in range(r * c)]
    return mock.MagicMock(), (axes[0] if r * c == 1 else axes)


mpl = mock.MagicMock()
mpl.pyplot.subplots = subplots
for name, m in (('matplotlib', mpl), ('matplotlib.pyplot', mpl.pyplot), ('matplotlib.gridspec', mpl.gridspec)):
    sys.modules[name] = m

os.chdir(REF)
g = runpy.run_path(os.path.join(REF, 'plot_act.py'), run_name='plot_act')
methods = list(g['methods'])

out = {'methods': np.array(methods), 'totals': np.array([c[-1] for c in g['IADC_cumsums']], np.float64)}
for name in ('QP', 'RL'):
    i = methods.index(name)
    for key, src in (('nbow', 'nbow'), ('nport', 'nport'), ('nstar', 'nstar'), ('aport', 'aport'), ('astar', 'astar'),
                     ('time_bow', 'time_bow'), ('time_stern', 'time_nstern')):
        out['%s_%s' % (name, key)] = np.asarray(g[src][i], np.float64).reshape(-1)
    for k in range(6):
        out['%s_derivs%d' % (name, k)] = np.asarray(g['derivs'][i][k], np.float64).reshape(-1)
    out['%s_IADC' % name] = np.asarray(g['IADC'][i], np.float64).reshape(-1)
    out['%s_IADC_cumsums' % name] = np.asarray(g['IADC_cumsums'][i], np.float64).reshape(-1)
    short = int((np.diff(out['%s_time_bow' % name])[1:] < 0.1).sum() + (np.diff(out['%s_time_stern' % name])[1:] < 0.1).sum())
    print('%-3s %5d bow / %5d stern samples, %4d intervals under 0.1 s, IADC (reference code) %.2f'
          % (name, len(out['%s_time_bow' % name]), len(out['%s_time_stern' % name]), short, out['%s_IADC_cumsums' % name][-1]))
np.savez_compressed(OUT, **out)
print('all four: %s; wrote %s (%d bytes)' % (', '.join('%s %.2f' % (m, t) for m, t in zip(methods, out['totals'])), OUT, os.path.getsize(OUT)))
