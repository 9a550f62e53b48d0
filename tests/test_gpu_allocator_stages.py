"""The allocation stage of a handle as the setters move it (include/dpenv.h: dpenv_set_dp_controller[_table], dpenv_set_qp_allocator[_table],
dpenv_set_nn_allocator).  A handle is in one of seven stages - controller off, pseudo-inverse, controller table, scalar QP, QP table with
and without scalar numbers held behind it, network - and every setter call, with and without NULL, is made from every one of them.  The
model below states what the library answers: a refusal (return code and the message's distinguishing words, the first of the checks that
fail) or the stage the handle is in afterwards.  A stage is told by what it flies: after the calls the handle is reset and flown, and its
obs / act / reward / done rows are those of a fresh handle configured directly into the predicted stage, bit for bit (same kernel, same
inputs).  dpenv_controller_label_qp[_ex] without numbers of their own then use the held ones, or refuse in the table's or the "no QP
allocator" wording.

Shape: 65 envs - a full wave plus one lane - and 3 steps."""
import math

import numpy as np
import pytest
import torch            # before anything loads libdpenv.so, as in every other GPU test module: the process then has one HIP runtime, torch's

from tests import helpers as H
from tests.test_nn_allocator_cpu import seeded_net

pytestmark = pytest.mark.gpu

N, T = 65, 3
ROWS = ('obs', 'act', 'rew', 'done')
OFF, PINV, CTAB, QPS, QPT, QPT_HELD, NN = 'off', 'pinv', 'ctab', 'qp', 'qp_table', 'qp_table+held', 'nn'
STAGES = (OFF, PINV, CTAB, QPS, QPT, QPT_HELD, NN)
CALLS = ('ctrl', 'ctrl_null', 'ctab', 'ctab_null', 'qp', 'qp_null', 'qptab', 'qptab_null', 'nn', 'nn_null')

EINVAL = r'error -1: '
CTRL_OFF = EINVAL + r'%s: the DP controller is off \(dpenv_set_dp_controller first\)'
NN_SET = EINVAL + r'%s: a neural allocator is set: the NN allocator runs with'
QP_SET = EINVAL + r'%s: the QP allocator runs with the DP controller on and its scalar numbers \(no per-env controller table\)'
NN_CTAB = EINVAL + r'dpenv_set_nn_allocator: a per-env controller table is in force: the NN allocator runs with'
NN_QP = EINVAL + r'dpenv_set_nn_allocator: a QP allocator is set: the NN allocator runs with'


def model(stage, call):
    """(refusal pattern or None, the stage afterwards): the transitions of include/dpenv.h, the refusal the FIRST failing check reports."""
    qp = stage in (QPS, QPT, QPT_HELD)
    if call == 'ctrl':                                   # controller on, scalar numbers: table, QP (held numbers included) and network go
        return None, PINV
    if call == 'ctrl_null':
        return None, OFF
    if call in ('ctab', 'ctab_null'):
        who = 'dpenv_set_dp_controller_table'
        if stage == OFF:
            return CTRL_OFF % who, stage
        if call == 'ctab_null':
            return None, PINV if stage == CTAB else stage
        if qp:
            return QP_SET % who, stage
        if stage == NN:
            return NN_SET % who, stage
        return None, CTAB
    if call in ('qp', 'qptab'):
        who = 'dpenv_set_qp_allocator' if call == 'qp' else 'dpenv_set_qp_allocator_table'
        if stage == OFF:
            return CTRL_OFF % who, stage
        if stage == NN:
            return NN_SET % who, stage
        if stage == CTAB:
            return QP_SET % who, stage
        if call == 'qp':
            return None, QPS
        return None, QPT_HELD if stage in (QPS, QPT_HELD) else QPT
    if call == 'qp_null':                                # drops the QP, the table and the held numbers
        return None, PINV if qp else stage
    if call == 'qptab_null':                             # back to the held numbers if any, else to the pseudo-inverse
        return None, {QPT: PINV, QPT_HELD: QPS}.get(stage, stage)
    if call == 'nn':
        if stage == OFF:
            return CTRL_OFF % 'dpenv_set_nn_allocator', stage
        if stage == CTAB:
            return NN_CTAB, stage
        if qp:
            return NN_QP, stage
        return None, NN
    if call == 'nn_null':
        return None, PINV if stage == NN else stage
    raise KeyError(call)


# ---- the numbers every handle of this module is configured with -------------------------------------------------------------------------
def _qp_params():
    from ml4ca_amd.deploy import qp_allocator_defaults
    return dict(qp_allocator_defaults(), iterations=4)


def _qp_table():
    from ml4ca_amd.deploy import qp_allocator_table
    base = _qp_params()
    k = np.arange(N)
    return H.to_dev(np.ascontiguousarray(qp_allocator_table(N, base, w_power=0.5 + 0.25 * (k % 4), f_max=base['f_max'] * (0.6 + 0.1 * (k % 3))[:, None])))


def _ctrl_table():
    from ml4ca_amd.deploy import dp_controller_defaults, dp_controller_table
    base = dp_controller_defaults()
    return H.to_dev(np.ascontiguousarray(dp_controller_table(N, base, kp=base['kp'] * (0.5 + 0.25 * (np.arange(N) % 5))[:, None])))


def _net():
    from ml4ca_amd.policy import nn_net_to
    return nn_net_to(dict(seeded_net((9, 20, 20, 6), seed=21, scale=3.0), leak=0.0), 'cuda:0')


QP_ITERS = 4


def apply(env, call):
    """One setter call through the Python layer; the table setters without the mask read-back (check=False: the rows are valid)."""
    if call == 'ctrl':
        env.set_dp_controller()
    elif call == 'ctrl_null':
        env.set_dp_controller(off=True)
    elif call == 'ctab':
        env.set_dp_controller_table(_ctrl_table(), check=False)
    elif call == 'ctab_null':
        env.set_dp_controller_table(None)
    elif call == 'qp':
        env.set_qp_allocator(_qp_params())
    elif call == 'qp_null':
        env.set_qp_allocator(off=True)
    elif call == 'qptab':
        env.set_qp_allocator_table(_qp_table(), iterations=QP_ITERS, check=False)
    elif call == 'qptab_null':
        env.set_qp_allocator_table(None)
    elif call == 'nn':
        env.set_nn_allocator(_net())
    elif call == 'nn_null':
        env.set_nn_allocator(off=True)
    else:
        raise KeyError(call)


# the shortest way into each stage on a fresh handle: "configured directly"
DIRECT = {OFF: (), PINV: ('ctrl',), CTAB: ('ctrl', 'ctab'), QPS: ('ctrl', 'qp'), QPT: ('ctrl', 'qptab'), QPT_HELD: ('ctrl', 'qp', 'qptab'),
          NN: ('ctrl', 'nn')}


def fresh(calls=()):
    """A handle with the current from 16 directions and `calls` made on it; not yet reset."""
    env = H.make_pair('final_cont', N, current=True, seed=5, auto_reset=True, terminate=True, max_ep_len=40)[0]
    beta = (2 * math.pi / 16) * (torch.arange(N, device=env.device) % 16).float()
    env.set_current(torch.full((N,), 0.2, device=env.device), beta.contiguous())
    for c in calls:
        apply(env, c)
    return env


def fly(env):
    """The handle's first reset (the config's seed: the same draw on every handle of this module), then one launch of T steps."""
    from ml4ca_amd.policy import controller_rollout
    env.reset()
    return {k: v.clone() for k, v in controller_rollout(env, T).items()}


_flights = {}


def flight_of(stage):
    """The rows a fresh handle configured directly into `stage` flies: computed once, shared, never written."""
    if stage not in _flights:
        _flights[stage] = fly(fresh(DIRECT[stage]))
    return _flights[stage]


def refused(fn, pattern):
    from ml4ca_amd import DpenvError
    with pytest.raises(DpenvError, match=pattern):
        fn()


def flies(env, stage, what):
    """The handle is in `stage`: it flies that stage's rows, and the label calls without numbers of their own answer as that stage does."""
    from ml4ca_amd.policy import controller_label_qp, controller_rollout
    if stage == OFF:
        env.reset()
        refused(lambda: controller_rollout(env, T), EINVAL + r'dpenv_controller_rollout: the DP controller is off')
        refused(lambda: controller_label_qp(env, flight_of(PINV)['obs']), EINVAL + r'dpenv_controller_label_qp: the DP controller is off')
        return
    out, want = fly(env), flight_of(stage)
    for k in ROWS:
        assert torch.equal(out[k], want[k]), '%s: %s differs from the %s flight in %d elements' % (what, k, stage, int((out[k] != want[k]).sum()))
    obs, flown = flight_of(PINV)['obs'], flight_of(PINV)['act']
    for who, kw, pass_q in (('dpenv_controller_label_qp', {}, 'pass q'), ('dpenv_controller_label_qp_ex', dict(flown=flown), 'pass q or qp_table')):
        if stage == QPS:                                 # the held numbers
            got, held = controller_label_qp(env, obs, cost=True, **kw), controller_label_qp(env, obs, params=_qp_params(), cost=True, **kw)
            for a, b in zip(got, held):
                assert torch.equal(a, b), '%s: %s does not label with the held numbers' % (what, who)
        elif stage in (QPT, QPT_HELD):
            refused(lambda: controller_label_qp(env, obs, **kw), EINVAL + who + r': a per-env QP table \(dpenv_set_qp_allocator_table\) is in force .*: ' + pass_q + '$')
        else:
            refused(lambda: controller_label_qp(env, obs, **kw), EINVAL + who + r': no QP allocator \(' + pass_q + ', or dpenv_set_qp_allocator first')


def test_the_stages_fly_different_rows():
    """What tells the stages apart below: the five allocations' act rows differ pairwise; the table with and without held numbers fly alike."""
    kinds = (PINV, CTAB, QPS, QPT, NN)
    for i, a in enumerate(kinds):
        assert bool(torch.isfinite(flight_of(a)['act']).all())
        for b in kinds[i + 1:]:
            assert not torch.equal(flight_of(a)['act'], flight_of(b)['act']), (a, b)
    assert torch.equal(flight_of(QPT)['act'], flight_of(QPT_HELD)['act'])


@pytest.mark.parametrize('call', CALLS)
def test_every_call_from_every_stage(call):
    """Each row of the transition table from each of the seven stages: refused with the stage left as it was, or accepted into the stage
    the model names."""
    for stage in STAGES:
        what = '%s from %s' % (call, stage)
        env = fresh(DIRECT[stage])
        pattern, after = model(stage, call)
        if pattern is None:
            apply(env, call)
        else:
            refused(lambda: apply(env, call), pattern)
        flies(env, after, what)


SEQUENCES = [
    (('ctrl', 'qp', 'qptab', 'qptab_null'), QPS),                       # QP -> QP table -> table(NULL) is the scalar QP flight
    (('ctrl', 'qptab', 'qptab_null'), PINV),                            # a QP table alone -> table(NULL) is the pseudo-inverse flight
    (('ctrl', 'qp', 'qp_null', 'nn'), NN),                              # QP -> QP(NULL) -> NN accepted
    (('ctrl', 'qp', 'qptab', 'qp_null', 'qptab_null'), PINV),           # QP(NULL) under a table drops the held numbers with it
    (('ctrl', 'qp', 'qptab', 'qp', 'qptab_null'), QPS),                 # the scalar setter replaces a table: nothing to return from
    (('ctrl', 'qp', 'qptab', 'ctrl'), PINV),                            # the controller set again drops every stage ...
    (('ctrl', 'qp', 'qptab', 'ctrl', 'qptab_null'), PINV),              # ... the held numbers included
    (('ctrl', 'nn', 'ctrl'), PINV),
    (('ctrl', 'ctab', 'ctrl'), PINV),
    (('ctrl', 'qp', 'qptab', 'ctrl_null', 'ctrl'), PINV),               # ... and so does off and on again
    (('ctrl', 'nn', 'ctrl_null', 'ctrl', 'qp'), QPS),
    (('ctrl', 'nn', 'nn_null', 'ctab'), CTAB),
    (('ctrl', 'ctab', 'ctab_null', 'qp', 'qptab'), QPT_HELD),
    (('ctrl', 'nn', 'qp_null', 'qptab_null', 'ctab_null'), NN),         # the NULL calls of the other setters leave a network alone
]


@pytest.mark.parametrize('calls,stage', SEQUENCES, ids=['-'.join(c) for c, _ in SEQUENCES])
def test_sequences(calls, stage):
    """Longer walks: every call is accepted, the model followed call by call names the stage, and the handle flies it."""
    at = OFF
    for c in calls:
        pattern, at = model(at, c)
        assert pattern is None
    assert at == stage
    flies(fresh(calls), stage, ' -> '.join(calls))


def test_refusals_inside_a_walk_leave_the_stage():
    """NN -> controller table refused; QP -> NN refused; table -> QP refused: the stage flown afterwards is the one before the call."""
    env = fresh(('ctrl', 'nn'))
    refused(lambda: apply(env, 'ctab'), NN_SET % 'dpenv_set_dp_controller_table')
    refused(lambda: apply(env, 'qp'), NN_SET % 'dpenv_set_qp_allocator')
    refused(lambda: apply(env, 'qptab'), NN_SET % 'dpenv_set_qp_allocator_table')
    flies(env, NN, 'NN after three refusals')
    env = fresh(('ctrl', 'qp', 'qptab'))
    refused(lambda: apply(env, 'nn'), NN_QP)
    refused(lambda: apply(env, 'ctab'), QP_SET % 'dpenv_set_dp_controller_table')
    apply(env, 'qptab_null')
    refused(lambda: apply(env, 'nn'), NN_QP)
    flies(env, QPS, 'the held numbers after the refusals')
    env = fresh(('ctrl', 'ctab'))
    refused(lambda: apply(env, 'qp'), QP_SET % 'dpenv_set_qp_allocator')
    refused(lambda: apply(env, 'nn'), NN_CTAB)
    flies(env, CTAB, 'the controller table after the refusals')


def test_the_order_of_the_refusals():
    """Two conditions failing at once: the message of the first check stands.  dpenv_set_qp_allocator: controller off, then a network set,
    then the numbers (qp_check), then the handle's configuration, then the table / per-env hulls."""
    bad = dict(_qp_params(), iterations=0)
    hulls = H.to_dev(H.random_hulls(np.random.RandomState(3), N))
    env = fresh()
    refused(lambda: env.set_qp_allocator(bad), CTRL_OFF % 'dpenv_set_qp_allocator')
    env = fresh(('ctrl', 'nn'))
    refused(lambda: env.set_qp_allocator(bad), NN_SET % 'dpenv_set_qp_allocator')
    refused(lambda: env.set_qp_allocator_table(_qp_table(), iterations=0, check=False), NN_SET % 'dpenv_set_qp_allocator_table')
    env = fresh(('ctrl', 'ctab'))
    env.set_vessel_params(hulls)
    refused(lambda: env.set_qp_allocator(bad), EINVAL + r'QP allocator: iterations')
    refused(lambda: env.set_qp_allocator_table(_qp_table(), iterations=0, check=False), EINVAL + r'QP allocator: iterations must be in 1\.\.32')
    refused(lambda: apply(env, 'qp'), QP_SET % 'dpenv_set_qp_allocator')
    refused(lambda: apply(env, 'qptab'), QP_SET % 'dpenv_set_qp_allocator_table')
    # per-env hulls alone refuse the QP setters in the same words; the network flies on them
    env = fresh(('ctrl',))
    env.set_vessel_params(hulls)
    refused(lambda: apply(env, 'qp'), QP_SET % 'dpenv_set_qp_allocator')
    refused(lambda: apply(env, 'qptab'), QP_SET % 'dpenv_set_qp_allocator_table')
    apply(env, 'nn')
    refused(lambda: env.set_nn_allocator(_net(), leak=1.5), EINVAL + r'.*leak')


@pytest.mark.parametrize('stage', [QPS, QPT, QPT_HELD])
def test_hulls_set_after_the_qp_are_refused_at_launch(stage):
    """The handle may change after the QP setter: per-env hull blocks then refuse the launch in the QP's words, and going back to the shared
    hull flies the stage again."""
    from ml4ca_amd.policy import controller_rollout
    env = fresh(DIRECT[stage])
    env.set_vessel_params(H.to_dev(H.random_hulls(np.random.RandomState(3), N)))
    env.reset()
    refused(lambda: controller_rollout(env, T), QP_SET % 'dpenv_controller_rollout' + r', on the shared hull or the thrust-loss preset \(no per-env hull blocks')
    env = fresh(DIRECT[stage])
    env.set_vessel_params(H.to_dev(H.random_hulls(np.random.RandomState(3), N)))
    env.set_vessel_params(None)
    flies(env, stage, 'hulls set and dropped under %s' % stage)


@pytest.mark.parametrize('calls,stage', [(('ctrl', 'qp'), QPS), (('ctrl', 'qptab'), QPT), (('ctrl', 'qp', 'qptab', 'qptab_null'), QPS),
                                         (('ctrl', 'qptab', 'qp'), QPS), (('ctrl', 'qp', 'qp_null', 'qptab'), QPT)])
def test_thruster_state_after_one_flight(calls, stage):
    """After a QP setter and one flight the thruster state is that of a fresh handle configured the same way and flown once; it is not at
    rest, and a setter that clears it does."""
    env, twin = fresh(calls), fresh(DIRECT[stage])
    fly(env), fly(twin)
    x = env.get_qp_allocator_state()
    assert torch.equal(x, twin.get_qp_allocator_state())
    assert float(x.abs().max()) > 0.0
    back = x.clone()
    env.set_qp_allocator_state(torch.zeros_like(x))
    assert float(env.get_qp_allocator_state().abs().max()) == 0.0
    env.set_qp_allocator_state(back)
    assert torch.equal(env.get_qp_allocator_state(), back)
    if stage == QPS:                                     # table(NULL) on the scalar stage: nothing changes, x stays
        apply(env, 'qptab_null')
        assert torch.equal(env.get_qp_allocator_state(), back)
    apply(env, 'qp')                                     # the scalar setter puts the thrusters at rest
    assert float(env.get_qp_allocator_state().abs().max()) == 0.0


def test_thruster_state_is_refused_without_a_qp():
    for stage in (OFF, PINV, CTAB, NN):
        env = fresh(DIRECT[stage])
        refused(env.get_qp_allocator_state, EINVAL + r'dpenv_get_qp_allocator_state: no QP allocator is set')
        refused(lambda: env.set_qp_allocator_state(torch.zeros((5, N), device=env.device)), EINVAL + r'dpenv_set_qp_allocator_state: no QP allocator is set')
    env = fresh(('ctrl', 'qp', 'qptab', 'qp_null'))
    refused(env.get_qp_allocator_state, EINVAL + r'dpenv_get_qp_allocator_state: no QP allocator is set')
