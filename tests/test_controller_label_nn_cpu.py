"""The network's labelling entry point without a GPU: dpenv_controller_label_nn is declared, exported and bound with the header's struct
layout; deploy.label_rows_nn, its host statement, against label_rows' z and BatchedNNAllocator row by row, in pieces and around done rows;
and the argument checks train.fit_nn_allocator makes of `init` before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_controller_label_qp_cpu import DT, _block, _same
from tests.test_nn_allocator_cpu import seeded_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = (((9, 20, 20, 20, 20, 6), 0.0), ((3, 17, 6), 0.2))


def _net(sizes, leak):
    return dict(seeded_net(sizes, seed=31 + sizes[1], scale=3.0), leak=leak)


def test_entry_point_is_declared_exported_and_bound():
    from ml4ca_amd import _lib, deploy, policy, train
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'dpenv.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bint\s+dpenv_controller_label_nn\s*\(', txt)
    assert hasattr(lib, 'dpenv_controller_label_nn') and 'dpenv_controller_label_nn' in _lib.SYMBOLS
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = [f[2] for f in (ln.split() for ln in nm.splitlines()) if len(f) == 3]
    assert 'dpenv_controller_label_nn' in exported
    assert not [s for s in exported if 'launch_controller_label_nn' in s], 'the cross-unit launcher stays out of the dynamic symbol table'
    version = int(re.search(r'#define DPENV_ABI_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.dpenv_abi_version() == 6
    assert lib.dpenv_controller_label_nn(None, None, None) == _lib.EINVAL              # no handle: refused, not crashed
    assert callable(policy.controller_label_nn) and callable(deploy.label_rows_nn)
    assert callable(train.nn_wrench_rows) and callable(train.fit_nn_allocator_on_policy)
    assert 'a labelling scan with the network' not in header                            # the NOT HERE sentence no longer lists it


def test_struct_layout_matches_header(tmp_path):
    from ml4ca_amd import _lib
    S = 'dpenv_controller_label_nn_io'
    fs = ('struct_size', 'T', 'obs', 'obs_dtype', 'done', 'z_in', 'z_out', 'act', 'raw', 'tau_out', 'a')
    items = ['sizeof(%s)' % S] + ['offsetof(%s, %s)' % (S, f) for f in fs]
    src = tmp_path / 'labnn.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpenv.h"\nint main(void){printf("%s\\n", %s);return 0;}\n' % (
        ' '.join(['%zu'] * len(items)), ', '.join('(size_t)' + it for it in items)))
    exe = tmp_path / 'labnn'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    A = _lib.ControllerLabelNnIO
    assert [name for name, _ in A._fields_] == list(fs)
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in fs]
    # the fields shared with dpenv_controller_label_io lie where that struct has them
    B = _lib.ControllerLabelIO
    assert all(getattr(A, f).offset == getattr(B, f).offset for f, _ in B._fields_)


@pytest.mark.parametrize('sizes,leak', NETS)
def test_label_rows_nn_is_label_rows_z_and_the_allocator_row_by_row(sizes, leak):
    from ml4ca_amd.deploy import BatchedDPController, BatchedNNAllocator, dp_controller_defaults, label_rows, label_rows_nn
    p, net = dp_controller_defaults(), _net(sizes, leak)
    obs, done, z0, _ = _block()
    T, n = done.shape
    act, z, raw, tau = label_rows_nn(p, net, obs, done, z0, dt=DT)
    assert act.dtype == raw.dtype == tau.dtype == z.dtype == np.float32
    assert act.shape == (T, n, 7) and raw.shape == (T, n, 6) and tau.shape == (T, n, 3) and z.shape == (3, n)
    _, wz = label_rows(p, obs, done, z0, dt=DT)                                         # the PID lines are label_rows'
    assert _same(z, wz)
    ctrl, alloc = BatchedDPController(n, p, dt=DT), BatchedNNAllocator(n, net)
    assert float(alloc.leak) == np.float32(leak)                                       # the net's leak is the allocator's
    ctrl.z = np.ascontiguousarray(z0.T)
    for t in range(T):
        wt = ctrl.wrench(obs[t])
        wa, wp = alloc.allocate(wt, raw=True)
        assert _same(tau[t], wt) and _same(act[t], wa) and _same(raw[t], wp), t
        ctrl.reset(done[t] != 0)
    assert np.isfinite(act).all() and np.abs(act[..., 0:3]).max() > 0.05
    assert (np.abs(tau) == np.asarray(p['tau_max'], np.float32)).any(), 'some wrench is clipped'
    # float64 is the same composition in the other arithmetic
    a64, z64, r64, t64 = label_rows_nn(p, net, obs, done, z0, dt=DT, dtype=np.float64)
    assert a64.dtype == np.float64 and np.abs(t64 - tau).max() < 1e-4 and np.abs(r64 - raw).max() < 1e-4
    # nn_params override the net's leak
    from ml4ca_amd.deploy import nn_allocator_params
    other, _, _, _ = label_rows_nn(p, net, obs, done, z0, dt=DT, nn_params=nn_allocator_params(net, leak=0.5))
    assert not np.array_equal(other, act)


@pytest.mark.parametrize('k', [1, 4, 8])
def test_label_rows_nn_in_pieces_equals_one_call(k):
    from ml4ca_amd.deploy import dp_controller_defaults, label_rows_nn
    p, net = dp_controller_defaults(), _net(*NETS[0])
    obs, done, z0, _ = _block(seed=6)
    T = obs.shape[0]
    one = label_rows_nn(p, net, obs, done, z0, dt=DT)
    a1, z, r1, t1 = label_rows_nn(p, net, obs[0:k], done[0:k], z0, dt=DT)
    a2, z, r2, t2 = label_rows_nn(p, net, obs[k:T], done[k:T], z, dt=DT)
    assert _same(np.concatenate([a1, a2]), one[0]) and _same(z, one[1])
    assert _same(np.concatenate([r1, r2]), one[2]) and _same(np.concatenate([t1, t2]), one[3])


def test_a_done_row_zeroes_z_behind_it_and_not_before():
    from ml4ca_amd.deploy import dp_controller_defaults, label_rows_nn
    p, net = dp_controller_defaults(), _net(*NETS[0])
    obs, done, z0, _ = _block()
    T, n = done.shape
    done[3, 1] = done[4, 1] = 1                                                        # env 1 flies near the setpoint: its wrench is never clipped
    obs[:, 2] = obs[:, 1]                                                              # ... and env 2, with done rows 3 and 4 too, is its twin
    z0[:, 2] = z0[:, 1]
    act, z, raw, tau = label_rows_nn(p, net, obs, done, z0, dt=DT)
    free = label_rows_nn(p, net, obs, None, z0, dt=DT)
    assert (np.abs(tau[:, 1]) < np.asarray(p['tau_max'], np.float32)).all()
    assert _same(tau[:, 2], tau[:, 1]) and _same(act[:, 2], act[:, 1])
    # env 2 has done rows 3 and 4: rows 0..3 are those of the block without done bytes (row 3 itself is labelled before its reset) ...
    assert _same(tau[:4, 2], free[3][:4, 2]) and _same(act[:4, 2], free[0][:4, 2])
    # ... row 4 is the chain from z = 0 on that row alone, and so is row 5 (two done rows in a row)
    for t in (4, 5):
        alone = label_rows_nn(p, net, obs[t:t + 1, 2:3], None, None, dt=DT)
        assert _same(alone[3][0, 0], tau[t, 2]) and _same(alone[0][0, 0], act[t, 2])
        assert not np.array_equal(free[3][t, 2], tau[t, 2])
    # env 3 has no done row: the block without done bytes throughout
    assert _same(tau[:, 3], free[3][:, 3]) and _same(z[:, 3], free[1][:, 3])
    # a done byte at the last row leaves z as 0; at row 0 it is rebuilt since
    assert done[T - 1, 1] != 0 and (z[:, 1] == 0).all() and done[0, 0] != 0 and (z[:, 0] != 0).any()
    # done=None is a block of zero done bytes, z=None is zeros
    zero = label_rows_nn(p, net, obs, np.zeros_like(done), z0, dt=DT)
    assert all(_same(u, v) for u, v in zip(free, zero))
    a = label_rows_nn(p, net, obs, done, None, dt=DT)
    b = label_rows_nn(p, net, obs, done, np.zeros_like(z0), dt=DT)
    assert all(_same(u, v) for u, v in zip(a, b)) and not np.array_equal(a[3], tau)
    with pytest.raises(ValueError):
        label_rows_nn(p, net, obs[..., :5], done, z0, dt=DT)
    with pytest.raises(ValueError):
        label_rows_nn(p, net, obs, done[:-1], z0, dt=DT)
    with pytest.raises(ValueError):
        label_rows_nn(p, net, obs, done, z0[:2], dt=DT)


def test_fit_nn_allocator_checks_init_before_it_touches_a_device():
    """Every refusal comes before the first tensor is moved: the device named here does not exist on the test machine's CPU side."""
    from ml4ca_amd import train as TR
    rng = np.random.RandomState(0)
    ds = dict(x=rng.normal(size=(8, 9)).astype(np.float32), tau=rng.normal(size=(8, 3)).astype(np.float32))
    P9, P3 = TR.layout(9, 6, True)['P'], TR.layout(3, 6, True)['P']
    assert P9 != P3
    kw = dict(iters=1, loss='wrench', device='meta')
    for bad in (np.zeros(P9 - 1, np.float32), np.zeros(P9 + 1, np.float32), np.zeros((1, P9), np.float32), np.zeros(P9, np.float64),
                np.zeros(P9, np.int32), np.zeros(P3, np.float32)):
        with pytest.raises(ValueError, match='init is a flat float32 theta'):
            TR.fit_nn_allocator(ds, in_dim=9, init=bad, **kw)
    with pytest.raises(ValueError, match='init is a flat float32 theta'):
        TR.fit_nn_allocator(ds, in_dim=3, init=np.zeros(P9, np.float32), **kw)
    import torch
    with pytest.raises(ValueError, match='init is a flat float32 theta'):
        TR.fit_nn_allocator(ds, in_dim=9, init=torch.zeros(P9, dtype=torch.float64), **kw)
    # the checks before it are what they were
    with pytest.raises(ValueError, match="loss must be"):
        TR.fit_nn_allocator(ds, init=np.zeros(P9, np.float32), loss='huber', device='meta')
    with pytest.raises(ValueError, match='reads the wrenches'):
        TR.fit_nn_allocator(dict(x=ds['x']), init=np.zeros(P9, np.float32), **kw)
    # nn_wrench_rows' own checks, and its rows on the CPU: one float32 product per entry
    from ml4ca_amd.deploy import nn_allocator_defaults
    tau = torch.as_tensor((rng.uniform(-1, 1, size=(33, 3)) * (69.0, 30.0, 80.0)).astype(np.float32))
    for in_dim in (9, 3):
        rows = TR.nn_wrench_rows(tau, in_dim)
        d = nn_allocator_defaults()
        ts = np.asarray(d['tau_scale'], np.float64).astype(np.float32)
        assert rows['tau'] is tau and tuple(rows['x'].shape) == (33, in_dim)
        assert np.array_equal(rows['x'].numpy()[:, -3:].view(np.uint32), (tau.numpy() * ts).view(np.uint32))
        if in_dim == 9:
            assert np.array_equal(rows['x'].numpy()[:, :6], np.broadcast_to(np.asarray(d['in_const'], np.float64).astype(np.float32), (33, 6)))
    for bad in (tau.double(), tau[:, :2], tau.numpy()):
        with pytest.raises(ValueError):
            TR.nn_wrench_rows(bad)
    with pytest.raises(ValueError):
        TR.nn_wrench_rows(tau, in_dim=6)
