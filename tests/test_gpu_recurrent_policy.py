"""
vs_step_policy with a recurrent policy (vs_set_policy_rnn): RNNPolicy / GRUPolicy / LSTMPolicy of P/policies/recurrent/rnn.py
evaluated inside the fused rollout kernel (k_rollout_rnn), their hidden state carried on the device from step to step and from
launch to launch, and what rollout() and ParallelRolloutSampler make of them.

What is checked, through the C-ABI (record mode 2, hidden-state record plane on, launches cut unevenly):
  * one step of the torch module on the recorded observation and the recorded hidden state BEFORE step t gives the recorded
    action and the recorded hidden state before step t + 1: |x - torch| <= 1e-5 (1 + |torch|) (printed with -s);
  * the hidden state is exactly 0 before the first step and before the first step after every auto-reset;
  * torch free-running from zero over the recorded observations gives the recorded actions (the kernel carries its own state);
  * vs_step fed with the recorded actions reproduces observations, states, rewards and done flags BIT FOR BIT;
  * one launch and eight launches give bit-identical records and final hidden states; the noise is N(0, 1) and never enters
    the hidden state.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KW = {"qq-su": dict(dt=0.004, max_steps=15), "qcp-su": dict(dt=0.002, max_steps=15), "qbb": dict(dt=0.01, max_steps=15),
      "pend": dict(dt=0.02, max_steps=15, init_state=np.array([0.1, 0.2]))}  # episodes end inside the 40 recorded steps
NL = {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid, None: None}
FAMILIES = ["qq-su", "qcp-su", "qbb", "pend"]


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def dev(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda()


def make_policy(vs, cell, hidden, layers, n_obs, n_act, out_nonlin=None, gain=1.0, seed=0):
    from simurlacra_amd.policies import GRUPolicy, LSTMPolicy, RNNPolicy
    from simurlacra_amd.spaces import BoxSpace, EnvSpec

    torch.manual_seed(seed)
    spec = EnvSpec(BoxSpace(-np.ones(n_obs), np.ones(n_obs)), BoxSpace(-np.ones(n_act), np.ones(n_act)))
    if cell in ("tanh", "relu"):
        pol = RNNPolicy(spec, hidden, layers, hidden_nonlin=cell, output_nonlin=NL[out_nonlin])
    else:
        pol = {"gru": GRUPolicy, "lstm": LSTMPolicy}[cell](spec, hidden, layers, output_nonlin=NL[out_nonlin])
    with torch.no_grad():
        pol.output_layer.weight.mul_(gain)
    return pol


def run_kernel(vs, name, pol, n, splits, auto_reset, idx=None, noise_std=None, noise_seed=0, seed=5):
    """a handle stepped by the policy in launches of `splits` steps; returns (records [T, n, ..], hidden before every step
    [T, n, H], final VS_POLICY_HIDDEN [n, H], the handle)"""
    from simurlacra_amd.policies import rnn_kernel_spec

    spec = rnn_kernel_spec(pol)
    assert spec is not None
    spec["noise_std"] = noise_std
    T = sum(splits)
    e = vs.VecSimEnv(name, n, **KW[name])
    e.set_auto_reset(auto_reset, seed=31)
    e.reset(seed=seed)
    e.set_policy_rnn(obs_idx=idx, **spec)
    e.set_record_mode(2)
    e.set_traj_capacity(T)
    e.set_policy_hidden_record(pol.hidden_size)
    t = 0
    for k in splits:
        e.set_traj_offset(t)
        e.step_policy(k, record=True, noise_seed=noise_seed)
        t += k
    tr = e.traj(T)
    hrec = e.hidden_record_tensor()[:T, :, :n].permute(0, 2, 1).cpu().numpy()
    hfin = e.policy_hidden()[:, :n].t().cpu().numpy()
    return tr, hrec, hfin, e


CASES = [(FAMILIES[k % 4], cell, hidden, layers)
         for k, (cell, hidden, layers) in enumerate((c, h, l) for c in ("tanh", "relu", "gru", "lstm") for l in (1, 2)
                                                     for h in (64, 24, 7))]


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_recurrent_kernel_against_torch_and_the_step_kernel(vs, case, auto_reset):
    L = vs._lib
    name, cell, hidden, layers = CASES[case]
    # one case with a partial observation, one with actions far beyond the action limits, some output nonlinearities
    idx = [0, 2, 4, 5] if case == 4 else None
    gain = 30.0 if case == 5 else 1.0
    out_nonlin = {7: "tanh", 10: "sigmoid", 13: "relu"}.get(case)
    n, splits = 300, (7, 13, 20)
    T = sum(splits)
    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    pol = make_policy(vs, cell, hidden, layers, len(idx) if idx else O, A, out_nonlin, gain, seed=case)
    H = pol.hidden_size
    tr, hrec, hfin, e = run_kernel(vs, name, pol, n, splits, auto_reset, idx=idx, seed=5 + case)
    done = tr["done"].astype(bool)  # [T, n]
    alive = np.ones((T, n), dtype=bool)  # steps that belong to a rollout (auto-reset off: up to the first done)
    if not auto_reset:
        alive[1:] = np.cumsum(done, axis=0)[:-1] == 0
    obs = tr["obs"] if idx is None else tr["obs"][..., idx]
    # (1) one step of torch on the records
    with torch.no_grad():
        act, hn = pol(torch.from_numpy(obs.reshape(T * n, -1).astype(np.float32)),
                      torch.from_numpy(hrec.reshape(T * n, H).astype(np.float32)))
    act, hn = act.numpy().reshape(T, n, A), hn.numpy().reshape(T, n, H)
    err_a = np.abs(tr["act"] - act) / (1.0 + np.abs(act))
    nxt = np.concatenate([hrec[1:], hfin[None]], axis=0)  # the hidden state before step t + 1 (the final one behind the last)
    carry = alive & ~done
    err_h = np.abs(nxt - hn) / (1.0 + np.abs(hn))
    print(f"{name} {cell} x{layers} {hidden} AR={auto_reset}: max |act - torch| / (1 + |torch|) = {err_a[alive].max():.2e}, "
          f"hidden {err_h[carry].max():.2e}; |act| up to {np.abs(act[alive]).max():.1f}")
    assert err_a[alive].max() < 1e-5
    assert err_h[carry].max() < 1e-5
    # (2) zero at the start and behind every auto-reset
    assert not hrec[0].any()
    if auto_reset:
        assert done[:-1].any()
        assert not hrec[1:][done[:-1]].any()
        assert not hfin[done[-1]].any()
    else:
        frozen = ~alive  # steps behind a lane's done: it keeps its hidden state
        assert np.array_equal(hrec[frozen], np.broadcast_to(hfin[None], hrec.shape)[frozen])
    # (3) torch free-running from zero over the recorded observations
    h = torch.zeros(n, H)
    worst = 0.0
    with torch.no_grad():
        for t in range(T):
            a, h = pol(torch.from_numpy(obs[t].astype(np.float32)), h)
            ok = alive[t]
            if ok.any():
                worst = max(worst, float((np.abs(tr["act"][t] - a.numpy()) / (1 + np.abs(a.numpy())))[ok].max()))
            if auto_reset:
                h[torch.from_numpy(done[t])] = 0.0
    print(f"    free-running: max |act - torch| / (1 + |torch|) = {worst:.2e}")
    assert worst < 1e-5  # measured: <= 2.9e-6
    # (4) the step: vs_step with the recorded actions from the same initial state, bit for bit
    ref = vs.VecSimEnv(name, n, **KW[name])
    ref.set_auto_reset(auto_reset, seed=31)
    ref.reset(seed=5 + case)
    lane = np.ones(n, dtype=bool)
    for t in range(T):
        assert np.array_equal(ref.get(L.VS_OBS)[lane], tr["obs"][t][lane]), (name, t)
        assert np.array_equal(ref.get(L.VS_STATE)[lane], tr["state"][t][lane]), (name, t)
        ref.step(dev(tr["act"][t]))
        assert np.array_equal(ref.get(L.VS_REW)[lane], tr["rew"][t][lane]), (name, t)
        assert np.array_equal(ref.get(L.VS_DONE).astype(bool)[lane], done[t][lane]), (name, t)
        if not auto_reset:
            lane &= ~done[t]
    for which in (L.VS_STATE, L.VS_STEPCOUNT, L.VS_RETURNS):
        assert np.array_equal(ref.get(which)[lane], e.get(which)[lane]), (name, which)
    assert e.error_count() == 0
    ref.close()
    e.close()


@pytest.mark.parametrize("cell,layers", [("gru", 2), ("lstm", 2), ("tanh", 1)])
def test_launch_cuts_are_bit_identical(vs, cell, layers):
    name = "qq-su"
    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    pol = make_policy(vs, cell, 24, layers, O, A, seed=11)
    a = run_kernel(vs, name, pol, 500, (40,), True)
    b = run_kernel(vs, name, pol, 500, (5,) * 8, True)
    for key in a[0]:
        assert np.array_equal(a[0][key], b[0][key]), key
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[0]["done"].any()
    a[3].close()
    b[3].close()


def test_recurrent_kernel_exploration_noise(vs):
    name, n, T = "qbb", 4096, 24
    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    pol = make_policy(vs, "gru", 32, 1, O, A, seed=3)
    H = pol.hidden_size
    std = np.array([0.3, 0.05], dtype=np.float32)
    a = run_kernel(vs, name, pol, n, (24,), True, noise_std=std, noise_seed=77)
    b = run_kernel(vs, name, pol, n, (5, 19), True, noise_std=std, noise_seed=77)
    for key in a[0]:
        assert np.array_equal(a[0][key], b[0][key]), key  # keyed by (env, episode, step), not by the launch
    assert np.array_equal(a[1], b[1])
    tr, hrec = a[0], a[1]
    with torch.no_grad():
        mean, hn = pol(torch.from_numpy(tr["obs"].reshape(T * n, O).astype(np.float32)),
                       torch.from_numpy(hrec.reshape(T * n, H).astype(np.float32)))
    z = (tr["act"] - mean.numpy().reshape(T, n, A)) / std
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and abs((z[..., 0] * z[..., 1]).mean()) < 0.01
    assert abs((z ** 3).mean()) < 0.03 and abs((z ** 4).mean() - 3.0) < 0.1
    # the noise never enters the hidden state: the noise-free module on the records gives the next recorded hidden state
    hn = hn.numpy().reshape(T, n, H)
    carry = ~tr["done"].astype(bool)[:-1]
    err = np.abs(hrec[1:] - hn[:-1]) / (1 + np.abs(hn[:-1]))
    assert err[carry].max() < 1e-5
    c = run_kernel(vs, name, pol, n, (24,), True, noise_std=std, noise_seed=78)
    assert not np.array_equal(c[0]["act"], tr["act"])  # another seed, another draw
    for x in (a, b, c):
        x[3].close()


def test_recurrent_kernel_argument_errors(vs):
    L = vs._lib
    import ctypes as C

    e = vs.VecSimEnv("qq-su", 64, **KW["qq-su"])
    lib, h = e._lib, e._h
    pol = make_policy(vs, "gru", 8, 1, 6, 1)
    p = pol.param_values.detach().numpy().astype(np.float32)
    ptr = p.ctypes.data_as(C.c_void_p)

    def desc(cell=L.VS_RNN_GRU, layers=1, hidden=8):
        d = L.RnnDesc()
        d.cell, d.n_layers, d.hidden = cell, layers, hidden
        return d

    assert lib.vs_set_policy_rnn(h, C.byref(desc()), ptr, p.size) == L.VS_OK
    assert lib.vs_set_policy_rnn(h, C.byref(desc(cell=4)), ptr, p.size) == L.VS_ERR_ARG
    assert lib.vs_set_policy_rnn(h, C.byref(desc(layers=0)), ptr, p.size) == L.VS_ERR_ARG
    assert lib.vs_set_policy_rnn(h, C.byref(desc(layers=3)), ptr, p.size) == L.VS_ERR_ARG
    assert lib.vs_set_policy_rnn(h, C.byref(desc(hidden=65)), ptr, p.size) == L.VS_ERR_ARG
    assert lib.vs_set_policy_rnn(h, C.byref(desc()), ptr, p.size - 1) == L.VS_ERR_ARG
    assert lib.vs_step_policy(h, 1, 0, 0) == L.VS_ERR_STATE  # (the refused calls removed the policy)
    e.set_act_pipeline(delay=1)
    assert lib.vs_set_policy_rnn(h, C.byref(desc()), ptr, p.size) == L.VS_ERR_STATE
    e.set_act_pipeline(delay=0)
    # one in-kernel policy at a time: a network replaces the recurrent policy and the other way round
    from simurlacra_amd.policies import rnn_kernel_spec

    e.set_policy_rnn(**rnn_kernel_spec(pol))
    assert lib.vs_get(h, L.VS_POLICY_HIDDEN)
    e.set_policy_fnn(np.zeros(6 * 8 + 8 + 8 + 1), [8], "tanh")
    assert not lib.vs_get(h, L.VS_POLICY_HIDDEN)
    e.step_policy(2)
    e.set_policy_rnn(p, "gru", 1, 8)
    e.step_policy(2)
    e.close()
    d = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=10)
    pd = make_policy(vs, "gru", 8, 1, 4, 1).param_values.detach().numpy().astype(np.float32)
    assert d._lib.vs_set_policy_rnn(d._h, C.byref(desc()), pd.ctypes.data_as(C.c_void_p), pd.size) == L.VS_ERR_ARG
    d.close()


def test_reset_zeroes_the_hidden_state(vs):
    name = "qq-su"
    pol = make_policy(vs, "lstm", 16, 2, 6, 1, seed=2)
    from simurlacra_amd.policies import rnn_kernel_spec

    e = vs.VecSimEnv(name, 128, **KW[name])
    e.set_policy_rnn(**rnn_kernel_spec(pol))
    e.step_policy(5)
    hid = e.policy_hidden()
    assert hid[:, :128].abs().sum() > 0
    mask = np.zeros(128, dtype=np.uint8)
    mask[:64] = 1
    e.reset(mask=mask, seed=1)
    h = hid[:, :128].cpu().numpy()
    assert not h[:, :64].any() and h[:, 64:].any()
    e.reset(seed=2)
    assert not hid[:, :128].cpu().numpy().any()
    e.close()


def test_rollout_with_a_recurrent_policy(vs):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=50)
    pol = vs.GRUPolicy(env.spec, 16, 1)
    ro = vs.rollout(env, pol, eval=True, seed=0)
    T = len(ro)
    assert ro.hidden_states.shape == (T, pol.hidden_size)
    assert not ro.hidden_states[0].any()
    h = pol.init_hidden()
    with torch.no_grad():
        for t in range(T):
            assert np.array_equal(ro.hidden_states[t], h.numpy())
            a, h = pol(torch.from_numpy(np.asarray(ro.observations[t])).to(torch.float32), h)
            assert np.array_equal(ro.actions[t], a.numpy())
    env.close()


@pytest.mark.parametrize("envname,cell", [("qq-su", "gru"), ("qcp-su", "lstm")])
def test_sampler_with_a_recurrent_policy(vs, envname, cell, monkeypatch):
    from simurlacra_amd.policies import NormalActNoiseExplStrat, rnn_kernel_spec

    cls = {"qq-su": vs.QQubeSwingUpSim, "qcp-su": vs.QCartPoleSwingUpSim}[envname]
    env = cls(dt=KW[envname]["dt"], max_steps=60)
    torch.manual_seed(0)
    policy = (vs.GRUPolicy if cell == "gru" else vs.LSTMPolicy)(env.spec, 24, 2)
    assert rnn_kernel_spec(policy) is not None
    calls = []
    orig = vs.VecSimEnv.step_policy
    monkeypatch.setattr(vs.VecSimEnv, "step_policy", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    fused = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=300, seed=4)
    ros_f = fused.sample()
    assert calls  # the fused path
    calls.clear()
    loop = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=300, seed=4, fuse_policy=False)
    ros_l = loop.sample()
    assert not calls
    graph = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=300, seed=4, fuse_policy=False, graph_policy=True)
    ros_g = graph.sample()
    assert len(ros_f) == len(ros_l) == len(ros_g) == 300
    pol = policy.to("cpu")
    H = pol.hidden_size
    worst = 0.0
    for rf, rl, rg in zip(ros_f, ros_l, ros_g):
        assert rf.hidden_states.shape == (len(rf), H) and rl.hidden_states.shape == (len(rl), H)
        assert not rf.hidden_states[0].any() and not rl.hidden_states[0].any()
        with torch.no_grad():
            want, _ = pol(torch.from_numpy(np.asarray(rf.observations[:-1], dtype=np.float32)),
                          torch.from_numpy(rf.hidden_states))
        worst = max(worst, float((np.abs(rf.actions - want.numpy()) / (1 + np.abs(want.numpy()))).max()))
        k = min(5, len(rf), len(rl))
        np.testing.assert_allclose(rf.observations[:k], rl.observations[:k], rtol=2e-4, atol=2e-5)
        # the captured graph replays the eager loop bit for bit
        assert np.array_equal(rg.observations, rl.observations) and np.array_equal(rg.actions, rl.actions)
        assert np.array_equal(rg.hidden_states, rl.hidden_states)
    assert worst < 1e-5
    # sample_packed() holds what sample() returns
    for smp, ros in ((vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=300, seed=4), ros_f),
                     (vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=300, seed=4, fuse_policy=False), ros_l)):
        (pk,) = smp.sample_packed()
        assert pk.hidden_states.shape == (pk.total + len(pk), H)
        for j in (0, 17, 299):
            ro = ros[j]
            assert np.array_equal(pk.hidden_states[pk.step_slice(j)].cpu().numpy(), ro.hidden_states)
            assert np.array_equal(pk.actions[pk.step_slice(j)].cpu().numpy(), ro.actions)
            assert not pk.hidden_states[pk.obs_slice(j)][-1].any()
    # an exploration wrapper keeps the fused path and the noise out of the hidden state
    noisy = NormalActNoiseExplStrat(policy, std_init=0.5)
    calls.clear()
    pol = policy.to("cpu")
    r_noise = vs.ParallelRolloutSampler(env, noisy, 1, min_rollouts=64, seed=4).sample()
    assert calls
    with torch.no_grad():
        for ro in r_noise[:8]:
            pol = policy.to("cpu")  # (the sampler may have moved it)
            _, hn = pol(torch.from_numpy(np.asarray(ro.observations[:-1], dtype=np.float32)), torch.from_numpy(ro.hidden_states))
            err = np.abs(hn.numpy()[:-1] - ro.hidden_states[1:]) / (1 + np.abs(hn.numpy()[:-1]))
            assert err.max() < 1e-5 if len(ro) > 1 else True
