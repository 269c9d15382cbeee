"""
One in-kernel policy per handle: whichever of vs_set_policy_fnn / _rnn / _linear / _playback comes next replaces the policy
that is set TOGETHER WITH its side state (population, rollout target, sensitivities, running hidden state), a NULL call of any
setter removes whatever kind is set, a refused call leaves what that setter's discipline says, and vs_destroy releases all of it.

Shapes: qq-su (O = 6, A = 1), 128 envs = two population groups of 64 lanes, exploration noise off.  Four small policies: an
FNN [8] tanh, a one-layer GRU of 8 units, a linear policy on ["identity", "sin"] and a playback table [3, 6, 1].  The references
are four recorded steps of every kind on a fresh handle; the per-kind test files hold each kind against torch or the oracle, so
everything here is bit-for-bit equality with those references.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAME, N, DT, O, A = "qq-su", 128, 0.004, 6, 1
KINDS = ["fnn", "rnn", "linear", "playback"]
LANE_SET = np.repeat(np.arange(2, dtype=np.int32), 64)
RNG = np.random.default_rng(7)
PARAMS = {"fnn": (0.5 * RNG.normal(size=O * 8 + 8 + 8 * A + A)).astype(np.float32),
          "rnn": (0.5 * RNG.normal(size=3 * 8 * O + 3 * 8 * 8 + 2 * 3 * 8 + 8 * A + A)).astype(np.float32),
          "linear": (0.5 * RNG.normal(size=A * 2 * O)).astype(np.float32)}
TABLE = (3.0 * RNG.normal(size=(3, 6, A))).astype(np.float32)
TARGET = RNG.normal(size=(3, 7, O)).astype(np.float32)


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def make(vs):
    return vs.VecSimEnv(NAME, N, DT)


def set_kind(e, kind):
    if kind == "fnn":
        e.set_policy_fnn(PARAMS["fnn"], [8], "tanh")
    elif kind == "rnn":
        e.set_policy_rnn(PARAMS["rnn"], "gru", 1, 8)
    elif kind == "linear":
        e.set_policy_linear(PARAMS["linear"], ["identity", "sin"])
    else:
        e.set_policy_playback(TABLE)


def set_kind_with_side_state(e, kind):
    """the policy and everything that belongs to it; returns whether its steps record (a population refuses record-off
    launches, sensitivities refuse records)"""
    set_kind(e, kind)
    if kind == "playback":
        e.set_rollout_target(TARGET)
        e.set_rollout_sens([0])
        return False
    if kind == "rnn":
        e.set_policy_hidden_record(8)
    e.set_policy_population(np.stack([PARAMS[kind], 0.5 * PARAMS[kind]]), LANE_SET)
    return True


def remove_by(e, kind):
    """the NULL call of that kind's setter"""
    if kind == "fnn":
        e.set_policy_fnn(None, None)
    elif kind == "rnn":
        e.set_policy_rnn(None)
    elif kind == "linear":
        e.set_policy_linear(None, None)
    else:
        e.set_policy_playback(None)


def four_steps(vs, e):
    """four recorded steps from reset(seed=1): the record's fields and the buffers the run leaves"""
    L = vs._lib
    e.reset(seed=1)
    e.set_traj_offset(0)
    e.step_policy(4, record=True)
    out = e.traj(4)
    out["VS_STATE"] = e.get(L.VS_STATE)
    out["VS_STEPCOUNT"] = e.get(L.VS_STEPCOUNT)
    return out


def assert_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def reference(vs):
    """{kind: four_steps of that kind on a fresh handle}; computed once, never written to"""
    ref = {}
    for kind in KINDS:
        e = make(vs)
        e.reset(seed=1)
        set_kind(e, kind)
        e.set_traj_capacity(8)
        ref[kind] = four_steps(vs, e)
        assert np.any(ref[kind]["act"] != 0), kind
        assert np.all(ref[kind]["VS_STEPCOUNT"] == 4), kind
        e.close()
    for a in range(4):
        for b in range(a):  # four policies, four records
            assert not np.array_equal(ref[KINDS[a]]["act"], ref[KINDS[b]]["act"])
    return ref


@pytest.mark.parametrize("k", KINDS)
@pytest.mark.parametrize("j", KINDS)
def test_a_new_policy_replaces_the_old_one_and_its_side_state(vs, reference, j, k):
    L = vs._lib
    e = make(vs)
    lib, h = e._lib, e._h
    e.set_traj_capacity(8)
    e.reset(seed=1)
    record = set_kind_with_side_state(e, j)
    e.step_policy(2, record=record)
    if j == "playback":
        assert lib.vs_get(h, L.VS_ROLLOUT_LOSS) and lib.vs_get(h, L.VS_ROLLOUT_GRAD)
    else:
        assert lib.vs_step_policy(h, 1, 0, 0) == L.VS_ERR_STATE  # (the population is there: no record-off launches)
    set_kind(e, k)
    assert_same(four_steps(vs, e), reference[k], (j, k))
    assert bool(lib.vs_get(h, L.VS_POLICY_HIDDEN)) == (k == "rnn")
    assert not lib.vs_get(h, L.VS_ROLLOUT_LOSS)  # the target and the sensitivities went with j
    assert not lib.vs_get(h, L.VS_ROLLOUT_GRAD)
    e.step_policy(1, record=False)  # ... and so did the population
    assert e.error_count() == 0
    e.close()


def test_a_null_call_of_any_setter_removes_any_kind(vs):
    L = vs._lib
    e = make(vs)
    for j in KINDS:
        for k in KINDS:
            set_kind(e, k)
            e.step_policy(1)
            remove_by(e, j)
            assert e._lib.vs_step_policy(e._h, 1, 0, 0) == L.VS_ERR_STATE, (j, k)
    e.close()


def lin_desc(vs):
    L = vs._lib
    d = L.LinDesc()
    d.n_terms = 2
    d.terms[0].kind, d.terms[1].kind = L.VS_FEAT_IDENTITY, L.VS_FEAT_SIN
    return d


def test_refused_linear_and_playback_calls_leave_the_network(vs, reference):
    L = vs._lib
    e = make(vs)
    lib, h = e._lib, e._h
    e.set_traj_capacity(8)
    set_kind(e, "fnn")
    p = PARAMS["linear"]
    assert lib.vs_set_policy_linear(h, C.byref(lin_desc(vs)), p.ctypes.data_as(C.c_void_p), p.size - 1) == L.VS_ERR_ARG
    assert lib.vs_set_policy_playback(h, TABLE.ctypes.data_as(C.c_void_p), 3, 0, None, None) == L.VS_ERR_ARG
    assert_same(four_steps(vs, e), reference["fnn"], "fnn behind two refused calls")
    e.close()


def test_refused_network_calls_remove_the_linear_policy(vs):
    L = vs._lib
    e = make(vs)
    lib, h = e._lib, e._h
    fd = L.FnnDesc()
    fd.n_hidden, fd.hidden[0], fd.hidden_nonlin[0] = 1, 65, L.VS_NL_TANH
    rd = L.RnnDesc()
    rd.cell, rd.n_layers, rd.hidden = L.VS_RNN_GRU, 3, 8
    pf, pr = PARAMS["fnn"], PARAMS["rnn"]
    for refused in (lambda: lib.vs_set_policy_fnn(h, C.byref(fd), pf.ctypes.data_as(C.c_void_p), pf.size),
                    lambda: lib.vs_set_policy_rnn(h, C.byref(rd), pr.ctypes.data_as(C.c_void_p), pr.size)):
        set_kind(e, "linear")
        e.step_policy(1)
        assert refused() == L.VS_ERR_ARG
        assert lib.vs_step_policy(h, 1, 0, 0) == L.VS_ERR_STATE
    e.close()


def test_create_and_destroy_with_every_kind_and_its_side_state(vs):
    L = vs._lib
    for _ in range(3):
        for kind in KINDS:
            e = make(vs)
            e.reset(seed=1)
            record = set_kind_with_side_state(e, kind)
            e.step_policy(2, record=record)
            e.sync()
            lib, h = e._lib, e._h
            e._h = None
            assert lib.vs_destroy(h) == L.VS_OK, kind
