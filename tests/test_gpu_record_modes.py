"""
The record mode of a fused rollout selects code inside the env step of every rollout kernel (REC in rollout_body, k_rollout_fnn
and k_rollout_rnn, three copies of the same statements): whether a launch records nothing, [obs | act | rew] (mode 1) or also
[state | act_app | hidden] (mode 2) must not change what the lanes do.

The same seeded batch runs three times -- unrecorded, mode 1, mode 2 -- through each of the three kernels: step_random pinned to
k_rollout, step_policy with a feed-forward network and step_policy with a GRU; with auto-reset off and on.  The lane buffers,
the episode statistics and (mode 1 against mode 2) the common record planes must be bit-identical.
130 lanes are two full waves and a mostly padded one; max_steps = 40 inside 50 steps cut (7, 1, 30, 12) ends every episode, and
restarts it under auto-reset, in the middle of a launch.  qq-su reuses the trig of its observation in the step, bob's action
bounds depend on its constants.

One leg is left out because the kernel differs there by design: VS_REW of
step_random without auto-reset, unrecorded against recorded.  An unrecorded wave leaves the step loop when its last lane has
ended (rollout_body's early exit) and keeps the last reward; a recording one goes on writing its frozen rows, and a frozen
lane's reward reads 0.  The two recorded runs are still compared with each other there.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, SPLITS = 130, (7, 1, 30, 12)
KW = {"qq-su": dict(dt=0.004, max_steps=40), "bob": dict(dt=0.01, max_steps=40)}
FNN_HIDDEN, GRU_HIDDEN = 16, 8


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def run(vs, name, caller, auto_reset, mode):
    """one batch, 50 steps in four launches; mode 0: unrecorded.  Returns (lane buffers, episode statistics, records)"""
    L = vs._lib
    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    rng = np.random.default_rng(3)
    e = vs.VecSimEnv(name, N, **KW[name])
    e.set_auto_reset(auto_reset, seed=31)
    e.reset(seed=5)
    if caller == "random":
        e.set_rollout_variant("k_rollout")
    elif caller == "fnn":
        h = FNN_HIDDEN
        e.set_policy_fnn(rng.uniform(-0.5, 0.5, O * h + h + h * A + A), [h], "tanh")
    else:
        h = GRU_HIDDEN
        e.set_policy_rnn(rng.uniform(-0.5, 0.5, 3 * h * O + 3 * h * h + 6 * h + h * A + A), "gru", 1, h)
    if mode:
        e.set_record_mode(mode)
        e.set_traj_capacity(sum(SPLITS))
    t = 0
    for k in SPLITS:
        if mode:
            e.set_traj_offset(t)
        if caller == "random":
            e.step_random(k, seed=9, record=bool(mode))
        else:
            e.step_policy(k, record=bool(mode))
        t += k
    e.sync()
    bufs = {w: e.get(getattr(L, w)) for w in ("VS_STATE", "VS_HIDDEN", "VS_OBS", "VS_STEPCOUNT", "VS_RETURNS", "VS_REW", "VS_DONE")}
    if caller == "gru":
        bufs["policy_hidden"] = e.policy_hidden()[:, :N].cpu().numpy()
    stats = e.episode_stats()
    tr = e.traj(sum(SPLITS)) if mode else None
    assert e.error_count() == 0
    e.close()
    return bufs, stats, tr


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("name", ["qq-su", "bob"])
@pytest.mark.parametrize("caller", ["random", "fnn", "gru"])
def test_record_mode_does_not_change_the_rollout(vs, caller, name, auto_reset):
    plain, rec1, rec2 = (run(vs, name, caller, auto_reset, mode) for mode in (0, 1, 2))
    assert plain[1][0].sum() > 0  # lanes finished
    if auto_reset:
        assert plain[0]["VS_STEPCOUNT"].max() < sum(SPLITS)  # and went on in a new episode
    early_exit = caller == "random" and not auto_reset  # (see the module docstring)
    for other in (rec1, rec2):
        for key in plain[0]:
            if key == "VS_REW" and early_exit:
                continue
            assert np.array_equal(plain[0][key], other[0][key]), key
        for x, y in zip(plain[1], other[1]):
            assert np.array_equal(x, y)
    assert np.array_equal(rec1[0]["VS_REW"], rec2[0]["VS_REW"])
    for key in ("obs", "act", "rew", "done"):
        assert np.array_equal(rec1[2][key], rec2[2][key]), key
    assert rec1[2]["done"].any()
