"""Are the edge tables of tests/step_edges.py fair?  (CPU only.)  The float32 oracle against the float64 oracle on tables A and B, through
the comparison the GPU test uses (step_edges.judge, floors of tests/tolerances.py unchanged, no row masked): the reference alone must stay
inside HALF the tolerance on every row - the convention of tests/tolerances.py, the kernel gets the other half.  Plus the oracle facts the
zero-head fix rests on.  The worst ratios are printed, and appended to the file the environment variable STEP_EDGES_RECORD names, if it is set
(profiles/step_edges_parity.txt is such a record)."""
import os

import numpy as np
import pytest

from tests import step_edges as SE

RECORD = os.environ.get('STEP_EDGES_RECORD')
HALF = 0.5


# every tag a table must hold, and how many rows of it at least: a row that float32 cannot hold is changed, never dropped
A_TAGS = {'full': {'component': 2 * 6 * 18}, 'simple': {'component': 2 * 3 * 18}, 'limited': {'component': 2 * 5 * 18},
          'final_wrap': {'component': 2 * (5 * 18 - 2 * 8), 'component_wrap_odd': 2 * 2 * 8, 'wrap_odd': 2 * 2 * 6, 'wrap_odd_nbr': 2 * 2 * 12,
                         'wrap_half': 2 * 2 * 24},
          'final_cont': {'component': 2 * 7 * 18, 'heads': 2 * 2 * 5 * 15, 'heads_seam': 2 * 2 * (5 + 2), 'heads_zero': 2 * 2 * 4,
                         'heads_unit': 2 * 2 * (2 + 4)}}
B_TAGS = {'heading': 27, 'fold': 2, 'heading_jump': 2, 'heading_jump_nbr': 4, 'heading_exact': 6, 'yaw_error': 16, 'yaw_error_jump': 4,
          'yaw_error_jump_nbr': 8, 'yaw_error_exact': 12}


def _tags(t, want):
    have = {tag: int((t.tag == tag).sum()) for tag in set(t.tag.tolist())}
    assert have == want, have


def _fair(t, od, n_substeps, steps, title):
    o32 = SE.make_oracle(t.mode, t.ext, np.float32, t.kw, n_substeps)
    o64 = SE.make_oracle(t.mode, t.ext, np.float64, t.kw, n_substeps)
    rows = SE.parity_rows(t)
    report, bad = SE.judge(SE.oracle_steps(o32, t, steps), SE.truth_variants(o64, t, steps), t, od, rows, limit=HALF)
    print(title, sorted(report.items()))
    SE.record(RECORD, 'float32 oracle / float64 oracle: ' + title, report)
    assert bad.size == 0, 'the float32 oracle itself misses half the tolerance: ' + '; '.join(SE.describe(t, i) for i in bad[:4])
    assert max(report.values()) <= HALF


@pytest.mark.parametrize('n_substeps', [20, 7])
@pytest.mark.parametrize('mode,ext', SE.ALL_CASES)
def test_table_a_is_fair(mode, ext, n_substeps):
    t = SE.table_a(mode, ext)
    assert 100 < t.n < SE.RAGGED // 2
    _tags(t, A_TAGS[mode])
    assert t.st.dtype == np.float32 and t.act.dtype == np.float32
    _fair(t, 9 if ext else 6, n_substeps, 1, 'A %s ext=%d substeps=%d' % (mode, ext, n_substeps))


@pytest.mark.parametrize('steps', [1, 3])
@pytest.mark.parametrize('n_substeps', [20, 7])
@pytest.mark.parametrize('wrap_mode', ['reference', 'radians'])
def test_table_b_is_fair(wrap_mode, n_substeps, steps):
    t = SE.table_b(wrap_mode)
    _tags(t, B_TAGS)                                  # the same rows in both wrap modes, and only |psi| > 30000 outside parity
    assert (~SE.parity_rows(t)).sum() == B_TAGS['fold']
    _fair(t, 9, n_substeps, steps, 'B %s substeps=%d steps=%d' % (wrap_mode, n_substeps, steps))


def test_padding_keeps_every_row_and_a_partial_last_workgroup():
    t = SE.table_a('final_cont', True)
    p = SE.padded(t, SE.moving_state('final_cont'), SE.mid_action('final_cont'))
    assert p.n == SE.RAGGED and p.n % 64 != 0
    edge = p.tag != 'pad'
    assert edge.sum() == t.n and edge[-1] and not (edge[1:] & edge[:-1]).any()
    assert p.st[:, edge].tobytes() == t.st.tobytes() and p.act[edge].tobytes() == t.act.tobytes() and (p.disc[edge] == t.disc).all()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_oracle_facts_of_zero_and_tiny_heads(dtype):
    """customEnv.py:227-235: the azimuth is numpy.arctan2 of the heads, the force follows THAT angle.  Full port thrust from rest:
    heads (0, +-0) push along +-surge, (-0, -0) along -surge at azimuth -pi, (1e-30, 0) along sway at azimuth pi/2."""
    t = SE.zero_head_fact_rows()
    o = SE.oracle_steps(SE.make_oracle('final_cont', True, dtype, t.kw), t)[0]
    u, v, az = o['st'][3], o['st'][4], o['st'][13]
    assert abs(u[0] - 0.01552) < 1e-5 and abs(u[1] + 0.01552) < 1e-5 and abs(u[2] + 0.01552) < 1e-5 and abs(u[3] - 0.01552) < 1e-5
    assert az[0] == 0 and abs(az[1] - np.pi) < 1e-6 and abs(az[2] + np.pi) < 1e-6 and az[3] == 0
    assert abs(az[4] - np.pi / 2) < 1e-6 and v[4] > 0.005 and abs(u[4]) < 0.01 * v[4]


def test_table_c_and_d_shapes():
    for mode, ext in SE.ALL_CASES:
        t = SE.table_c(mode, ext)
        assert t.n == 1 + 6 * 6 and (t.st[2][t.tag != 'inside'][:12] == 0).all()
    n_pct, alpha, which = SE.table_d()
    assert n_pct.shape == alpha.shape and n_pct.shape[0] == 3 and n_pct.dtype == np.float32
    assert (np.abs(n_pct).sum(0) == 100).all()
    bow = (which == 0) & (alpha[0] == np.float32(np.pi / 2))
    assert bow.sum() == 2                                        # the special-cased constant of the bow thruster, both thrust signs
