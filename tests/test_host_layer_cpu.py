"""The host labelling scan shared by deploy.label_rows, label_rows_qp and label_rows_nn (deploy._label_scan): the PID half of the three
is one code path, so the z they return is the same bits, and a block labelled in two pieces with z (and x) handed over is the block
labelled in one."""
import numpy as np

from tests.test_controller_label_qp_cpu import DT, _qp, _same
from tests.test_nn_allocator_cpu import seeded_net

T, N = 3, 2


def _block():
    """T = 3 rows of n = 2 envs in float32: done bytes at row 0 (env 0) and at the last row (env 1), a non-zero starting z and x."""
    rng = np.random.RandomState(12)
    obs = (rng.uniform(-1.0, 1.0, (T, N, 9)) * (6, 6, 1.5, 1, 0.5, 0.4, 1, 1, 1)).astype(np.float32)
    done = np.zeros((T, N), np.uint8)
    done[0, 0] = 1
    done[T - 1, 1] = 2
    z0 = rng.uniform(-0.5, 0.5, (3, N)).astype(np.float32)
    x0 = (rng.uniform(-1.0, 1.0, (5, N)) * np.array([4, 8, 8, 2, 2])[:, None]).astype(np.float32)
    assert (z0 != 0).all()
    return obs, done, z0, x0


def _callers():
    """(name, label(obs, done, z, x) -> (act, z, x or None, further outputs)) for the three host statements."""
    from ml4ca_amd.deploy import dp_controller_defaults, label_rows, label_rows_nn, label_rows_qp
    p, q = dp_controller_defaults(), _qp()
    net = dict(seeded_net((9, 20, 20, 6), seed=7, scale=3.0), leak=0.2)

    def pinv(obs, done, z, x):
        act, z = label_rows(p, obs, done, z, dt=DT)
        return act, z, None, ()

    def qp(obs, done, z, x):
        act, z, x = label_rows_qp(p, q, obs, done, z, x, dt=DT)
        return act, z, x, ()

    def nn(obs, done, z, x):
        act, z, raw, tau = label_rows_nn(p, net, obs, done, z, dt=DT)
        return act, z, None, (raw, tau)

    return (('label_rows', pinv), ('label_rows_qp', qp), ('label_rows_nn', nn))


def test_the_three_scans_return_the_same_z_bit_for_bit():
    obs, done, z0, x0 = _block()
    zs = [label(obs, done, z0, x0)[1] for _, label in _callers()]
    assert zs[0].dtype == np.float32 and zs[0].shape == (3, N)
    assert _same(zs[0], zs[1]) and _same(zs[0], zs[2])
    assert (zs[0][:, 1] == 0).all() and (zs[0][:, 0] != 0).any()          # done at the last row leaves 0; at row 0, z is rebuilt since


def test_two_pieces_with_the_state_handed_over_equal_one_call():
    obs, done, z0, x0 = _block()
    k = 1
    for name, label in _callers():
        act, z, x, more = label(obs, done, z0, x0)
        a1, z1, x1, m1 = label(obs[:k], done[:k], z0, x0)
        a2, z2, x2, m2 = label(obs[k:], done[k:], z1, x1)
        assert act.shape == (T, N, 7) and act.dtype == np.float32, name
        assert _same(np.concatenate([a1, a2]), act), name
        assert _same(z2, z), name
        assert x is None or _same(x2, x), name
        assert all(_same(np.concatenate([u, v]), w) for u, v, w in zip(m1, m2, more)), name
