"""
A population of policy parameter vectors in one fused launch (vs_set_policy_population) and ParameterExploringSampler on top.

What is checked:
  * kernel identity: every set's records (observations, actions, rewards, done bits, lengths; the hidden-state records of a
    recurrent policy) are BIT-IDENTICAL to a single-policy vs_step_policy run with that set's vector on the same lanes, shape and
    seeds -- FNN of 1-4 hidden layers in the 64-env, 256-env and matrix-core shapes, RNN tanh / relu, GRU and LSTM of 1-2
    layers, one case with exploration noise; sets really differ (a kernel that reads set 0 everywhere fails);
  * inert (-1) groups: length 0, no state change, no record row written, also after a vs_reset; the refusals;
  * the sampler: fused population == the fuse_policy=False loop, == ParallelRolloutSampler per set, padding and batch cuts
    invisible, the same seed bit-identical.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KW = {"qq-su": dict(dt=0.004, max_steps=50), "qcp-su": dict(dt=0.002, max_steps=50)}


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def fnn_sets(vs, name, hidden, P, seed, gain=10.0):
    from simurlacra_amd.policies import FNN

    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    torch.manual_seed(seed)
    out = []
    for _ in range(P):
        net = FNN(O, A, list(hidden), torch.tanh)
        with torch.no_grad():
            net.output_layer.weight.mul_(gain)
        out.append(torch.nn.utils.parameters_to_vector(net.parameters()).detach())
    return torch.stack(out)


def rnn_policy(vs, name, cell, hidden, layers, seed):
    from simurlacra_amd.policies import GRUPolicy, LSTMPolicy, RNNPolicy
    from simurlacra_amd.spaces import BoxSpace, EnvSpec

    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    torch.manual_seed(seed)
    spec = EnvSpec(BoxSpace(-np.ones(O), np.ones(O)), BoxSpace(-np.ones(A), np.ones(A)))
    if cell in ("tanh", "relu"):
        return RNNPolicy(spec, hidden, layers, hidden_nonlin=cell)
    return {"gru": GRUPolicy, "lstm": LSTMPolicy}[cell](spec, hidden, layers)


def run(vs, name, n, set_policy, splits, rec_mode=2, shape=None, population=None, hidden_rec=0, noise_seed=3, seed=5):
    """one handle: policy, optional population, launches of `splits` steps; returns (traj dict, lengths, hidden records, handle)"""
    e = vs.VecSimEnv(name, n, **KW[name])
    e.reset(seed=seed)
    set_policy(e)
    if population is not None:
        e.set_policy_population(*population)
    e.set_policy_shape(shape)
    e.set_record_mode(rec_mode)
    T = sum(splits)
    e.set_traj_capacity(T)
    if hidden_rec:
        e.set_policy_hidden_record(hidden_rec)
    t = 0
    for k in splits:
        e.set_traj_offset(t)
        e.step_policy(k, record=True, noise_seed=noise_seed)
        t += k
    tr = {k: v.cpu().numpy() for k, v in e.traj_tensors(T, n).items() if v is not None}
    length, _ = e.rollout_lengths(n, T)
    hrec = e.hidden_record_tensor()[:T, :, :n].cpu().numpy() if hidden_rec else None
    return tr, length.cpu().numpy(), hrec, e


def assert_same_lanes(a, b, lanes, what):
    tr_a, len_a, h_a = a[:3]
    tr_b, len_b, h_b = b[:3]
    for k in tr_a:
        if k == "rec":
            continue
        assert np.array_equal(tr_a[k][:, lanes], tr_b[k][:, lanes]), (what, k)
    assert np.array_equal(len_a[lanes], len_b[lanes]), what
    if h_a is not None:
        assert np.array_equal(h_a[:, :, lanes], h_b[:, :, lanes]), (what, "hidden")


FNN_CASES = [  # family, hidden sizes, shape, record mode, noise
    ("qq-su", (64,), "64", 2, None), ("qcp-su", (64,), "256", 1, None), ("qq-su", (64,), "mfma", 2, None),
    ("qcp-su", (64, 64), "64", 2, None), ("qq-su", (64, 64), "256", 2, None), ("qcp-su", (64, 64), "mfma", 1, None),
    ("qq-su", (24, 17), None, 2, None), ("qcp-su", (32, 16, 8), None, 2, None), ("qq-su", (16, 16, 16, 16), None, 1, None),
    ("qq-su", (64, 64), "mfma", 2, 0.4),
]


@pytest.mark.parametrize("case", range(len(FNN_CASES)))
def test_fnn_population_is_bit_identical_to_single_runs(vs, case):
    name, hidden, shape, rec, noise = FNN_CASES[case]
    P, n, splits = 3, 1024, (37, 40)
    sets = fnn_sets(vs, name, hidden, P, seed=case)
    lane_set = np.repeat(np.arange(4) % P, 256).astype(np.int32)  # uniform in groups of 256: every shape
    kw = dict(hidden_sizes=hidden, noise_std=noise)
    pop = run(vs, name, n, lambda e: e.set_policy_fnn(sets[0], **kw), splits, rec, shape, population=(sets.cuda(), lane_set))
    singles = [run(vs, name, n, lambda e, s=s: e.set_policy_fnn(sets[s], **kw), splits, rec, shape) for s in range(P)]
    for s in range(P):
        assert_same_lanes(pop, singles[s], np.flatnonzero(lane_set == s), (case, s))
    # the sets really differ: set 1's lanes do not act like set 0's vector
    lanes1 = np.flatnonzero(lane_set == 1)
    assert not np.array_equal(pop[0]["act"][:, lanes1], singles[0][0]["act"][:, lanes1])
    assert pop[0]["done"].any()
    for r in [pop] + singles:
        assert r[3].error_count() == 0
        r[3].close()


def test_fnn_population_in_groups_of_64(vs):
    """a table that is uniform in groups of 64 only: the automatic shape falls back to 64-env workgroups (the single-policy run
    for two narrow layers takes the matrix-core shape: compared with shape 64 pinned); a pinned 256-env shape is refused"""
    name, hidden, P, n, splits = "qq-su", (32, 24), 5, 1024, (50, 27)
    sets = fnn_sets(vs, name, hidden, P, seed=9)
    lane_set = np.repeat(np.array([0, 3, 1, 4, 2, 0, 1, 2, 3, 4, 4, 2, 1, 0, 3, 1]), 64).astype(np.int32)
    kw = dict(hidden_sizes=hidden)
    vs_shape_auto = run(vs, name, n, lambda e: e.set_policy_fnn(sets[0], **kw), splits, 2, None, population=(sets, lane_set))
    for s in range(P):
        single = run(vs, name, n, lambda e: e.set_policy_fnn(sets[s], **kw), splits, 2, "64")
        assert_same_lanes(vs_shape_auto, single, np.flatnonzero(lane_set == s), s)
        single[3].close()
    e = vs_shape_auto[3]
    for shape in ("256", "mfma"):
        e.set_policy_shape(shape)
        e.set_traj_offset(0)
        with pytest.raises(RuntimeError, match=r"\(-3\).*256"):
            e.step_policy(5, record=True)
    e.close()


RNN_CASES = [("qq-su", "tanh", 24, 1), ("qcp-su", "relu", 7, 2), ("qq-su", "gru", 64, 1), ("qcp-su", "gru", 24, 2),
             ("qq-su", "lstm", 24, 1), ("qcp-su", "lstm", 17, 2)]


@pytest.mark.parametrize("case", range(len(RNN_CASES)))
def test_rnn_population_is_bit_identical_to_single_runs(vs, case):
    from simurlacra_amd.policies import rnn_kernel_spec

    name, cell, hidden, layers = RNN_CASES[case]
    P, n, splits = 3, 512, (30, 41)
    pols = [rnn_policy(vs, name, cell, hidden, layers, seed=10 * case + s) for s in range(P)]
    specs = [rnn_kernel_spec(p) for p in pols]
    sets = torch.stack([sp["params"] for sp in specs])
    H = pols[0].hidden_size
    lane_set = np.repeat(np.array([2, 0, 1, 1, 0, 2, 2, 0]), 64).astype(np.int32)
    noise = 0.3 if case == 2 else None

    def setter(s):
        def f(e):
            sp = dict(specs[s])
            sp["noise_std"] = noise
            e.set_policy_rnn(**sp)
        return f

    pop = run(vs, name, n, setter(0), splits, 2, population=(sets, lane_set), hidden_rec=H)
    for s in range(P):
        single = run(vs, name, n, setter(s), splits, 2, hidden_rec=H)
        lanes = np.flatnonzero(lane_set == s)
        assert_same_lanes(pop, single, lanes, (case, s))
        assert np.array_equal(pop[3].policy_hidden()[:, lanes].cpu().numpy(), single[3].policy_hidden()[:, lanes].cpu().numpy())
        if s == 1:
            assert not np.array_equal(pop[0]["act"][:, np.flatnonzero(lane_set == 0)], single[0]["act"][:, np.flatnonzero(lane_set == 0)])
        single[3].close()
    pop[3].close()


@pytest.mark.parametrize("kind", ["fnn", "gru"])
def test_inert_groups_and_refusals(vs, kind):
    L = vs._lib
    name, n, T = "qq-su", 512, 40
    if kind == "fnn":
        sets = fnn_sets(vs, name, (32, 32), 2, seed=1)

        def setter(e):
            e.set_policy_fnn(sets[0], hidden_sizes=(32, 32))
    else:
        from simurlacra_amd.policies import rnn_kernel_spec

        specs = [rnn_kernel_spec(rnn_policy(vs, name, "gru", 16, 1, seed=s)) for s in range(2)]
        sets = torch.stack([sp["params"] for sp in specs])

        def setter(e):
            e.set_policy_rnn(**specs[0])
    e = vs.VecSimEnv(name, n, **KW[name])
    e.reset(seed=2)
    setter(e)
    e.set_record_mode(2)
    e.set_traj_capacity(T)
    e.step_policy(T, record=True)  # fills every lane's record rows
    before = {k: v.cpu().numpy().copy() for k, v in e.traj_tensors(T, n).items() if v is not None}
    e.reset(seed=3)
    inert = np.zeros(n, dtype=bool)
    inert[64:128] = inert[384:512] = True  # a 64-group and a whole 128-lane stretch
    lane_set = np.where(inert, -1, np.repeat(np.arange(8) % 2, 64)).astype(np.int32)
    e.set_policy_population(sets, lane_set)
    for rnd in range(2):  # ... and again after a vs_reset: the table stays
        st0 = e.get(L.VS_STATE).copy()
        steps0 = e.get(L.VS_STEPCOUNT).copy()
        e.set_traj_offset(0)
        e.step_policy(T, record=True)
        length, done_last = e.rollout_lengths(n, T)
        length, done_last = length.cpu().numpy(), done_last.cpu().numpy()
        assert (length[inert] == 0).all() and not done_last[inert].any()
        assert (length[~inert] > 0).all()
        assert np.array_equal(e.get(L.VS_STATE)[inert], st0[inert])  # not stepped
        assert np.array_equal(e.get(L.VS_STEPCOUNT)[inert], steps0[inert])
        assert not np.array_equal(e.get(L.VS_STATE)[~inert], st0[~inert])
        after = {k: v.cpu().numpy() for k, v in e.traj_tensors(T, n).items() if v is not None}
        for k in after:  # an inert lane's record rows keep what was there: nothing is written for it
            if k != "rec":
                assert np.array_equal(after[k][:, inert], before[k][:, inert]), k
        e.reset(seed=4 + rnd)
    # refusals
    bad = lane_set.copy()
    bad[70] = 0  # a mixed group of 64
    with pytest.raises(vs.ValueErr, match="64"):
        e.set_policy_population(sets, bad)
    with pytest.raises(vs.ValueErr):
        e.set_policy_population(sets[:, :-1], lane_set)  # parameter count
    with pytest.raises(vs.ValueErr):
        e.set_policy_population(sets, np.where(lane_set == 1, 2, lane_set))  # set id >= n_sets
    e.set_auto_reset(True, seed=1)
    with pytest.raises(RuntimeError, match=r"\(-3\).*-1 lanes"):
        e.step_policy(4, record=True)
    e.set_auto_reset(False)
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        e.step_policy(4, record=False)
    # setting a policy drops the population: auto-reset runs again
    setter(e)
    e.set_auto_reset(True, seed=1)
    e.step_policy(4, record=True)
    e.set_policy_fnn(None, None)
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        e.set_policy_population(sets, lane_set)  # no policy
    e.close()


# ------------------------------------------------------------------------------------------------ the sampler
def make_policy(vs, kind, env, seed=0):
    torch.manual_seed(seed)
    if kind == "fnn":
        return vs.FNNPolicy(env.spec, [64, 64], torch.tanh)
    return vs.GRUPolicy(env.spec, 16, 1)


def population(policy, P, seed):
    torch.manual_seed(seed)
    p0 = policy.param_values.detach()
    return torch.stack([p0 + 0.3 * torch.randn_like(p0) for _ in range(P)])


@pytest.mark.parametrize("kind", ["fnn", "gru"])
def test_sampler_against_the_loop_and_the_rollout_sampler(vs, kind, monkeypatch):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=120)
    policy = make_policy(vs, kind, env)
    P = 3
    params = population(policy, P, seed=1)
    calls = []
    orig = vs.VecSimEnv.set_policy_population
    monkeypatch.setattr(vs.VecSimEnv, "set_policy_population", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    for R in (10, 70):
        np.random.seed(R)
        inits = [env.init_space.sample_uniform() for _ in range(R)]
        fused = vs.ParameterExploringSampler(env, policy, R, 1, seed=2)
        res = fused.sample(params, init_states=inits)
        assert calls  # the population path
        calls.clear()
        assert len(res) == P and res.num_rollouts == P * R and all(s.num_rollouts == R for s in res)
        assert torch.equal(res.parameters, params)
        loop = vs.ParameterExploringSampler(env, policy, R, 1, seed=2, fuse_policy=False)
        res_l = loop.sample(params, init_states=inits)
        assert not calls
        for s in range(P):
            # the ParallelRolloutSampler with that set's vector: bit for bit (no noise, same kernel shape and lanes' inputs)
            pol_s = make_policy(vs, kind, env)
            pol_s.param_values = params[s]
            ros = vs.ParallelRolloutSampler(env, pol_s, 1, min_rollouts=R, seed=2).sample(init_states=inits)
            for a, b, c in zip(res[s].rollouts, ros, res_l[s].rollouts):
                assert np.array_equal(a.observations, b.observations) and np.array_equal(a.actions, b.actions)
                assert np.array_equal(a.rewards, b.rewards) and np.array_equal(a.states, b.states)
                assert np.array_equal(a.observations[0], np.asarray(c.observations[0], dtype=a.observations.dtype))
                assert len(a) == len(c)
                k = min(5, len(a))
                np.testing.assert_allclose(a.observations[:k], c.observations[:k], rtol=2e-4, atol=2e-5)
            assert res[s].mean_undiscounted_return == pytest.approx(res_l[s].mean_undiscounted_return, rel=1e-2)
        fused.close()
        loop.close()
    assert torch.equal(policy.param_values, make_policy(vs, kind, env).param_values)  # the loop restored the policy


@pytest.mark.parametrize("kind", ["fnn", "gru"])
def test_sampler_batches_seeds_and_domains(vs, kind):
    from simurlacra_amd.policies import NormalActNoiseExplStrat

    base = vs.QQubeSwingUpSim(dt=0.004, max_steps=100)
    env = vs.DomainRandWrapperLive(base, vs.create_default_randomizer(base))
    policy = NormalActNoiseExplStrat(make_policy(vs, kind, base), std_init=0.3)
    params = population(policy.policy, 5, seed=3)

    def sample(**kw):
        np.random.seed(7)
        torch.manual_seed(7)  # (the randomizer draws from torch's generator)
        smp = vs.ParameterExploringSampler(env, policy, 7, 3, **kw)
        out = smp.sample(params)
        smp.close()
        return out

    one = sample(seed=11)
    cut = sample(seed=11, batch_lanes=128)  # stride 64: two sets per batch, three batches
    again = sample(seed=11)
    other = sample(seed=12)
    assert one.num_rollouts == 5 * 21
    for a, b, c, d in zip(one, cut, again, other):
        for ra, rb, rc, rd in zip(a.rollouts, b.rollouts, c.rollouts, d.rollouts):
            for x in (rb, rc):
                assert np.array_equal(ra.observations, x.observations) and np.array_equal(ra.actions, x.actions)
                assert np.array_equal(ra.rewards, x.rewards)
            assert np.array_equal(ra.observations[0], rd.observations[0])  # (same NumPy draws)
        assert any(not np.array_equal(ra.actions, rd.actions) for ra, rd in zip(a.rollouts, d.rollouts))  # another noise key
    # common random numbers: every set sees the same domains (outer) and init states (inner)
    dp = [[ro.rollout_info["domain_param"] for ro in s.rollouts] for s in one]
    x0 = [[ro.observations[0] for ro in s.rollouts] for s in one]
    for s in range(1, 5):
        assert dp[s] == dp[0]
        assert all(np.array_equal(a, b) for a, b in zip(x0[s], x0[0]))
    assert dp[0][0] == dp[0][6] and dp[0][0] != dp[0][7]  # domain outer, 7 init states inner
    assert np.array_equal(x0[0][0], x0[0][7]) and not np.array_equal(x0[0][0], x0[0][1])
