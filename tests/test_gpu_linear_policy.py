"""
vs_step_policy with a linear policy on a feature stack (vs_set_policy_linear, k_rollout_lin): LinearPolicy(spec, FeatureStack(..))
of upstream Pyrado policies/feed_forward/linear.py over policies/features.py, evaluated inside the fused rollout kernel.

What is checked, through the C-ABI:
  * the recorded action of every step against the definitions of the feature functions, evaluated in fp64 NumPy on the recorded
    fp32 observation: |act - ref| <= 1e-5 (1 + sum_k |w_k phi_k|) -- the project's contract for an in-kernel policy in fp32 with
    another summation order, on the sum of absolute terms because a linear map of cubic and signed features cancels (128 fp32
    roundings are 7.6e-6 of that sum, sincos_fast adds <= 4e-7 absolute per feature); the worst ratio is printed with -s
    (DESIGN.md section 4 keeps the measured figure; not measured yet when this file was written);
  * everything else is the step kernel's: vs_step fed the recorded actions from the same initial state reproduces the recorded
    observations, states, rewards and done bits BIT FOR BIT (with and without auto-reset, launches cut unevenly);
  * launch cuts, exploration noise, populations (with an inert group), the refusals, and the two samplers.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from simurlacra_amd import features as F  # noqa: E402
from simurlacra_amd.policies import LinearPolicy, NormalActNoiseExplStrat, linear_kernel_spec  # noqa: E402
from simurlacra_amd.spaces import BoxSpace, EnvSpec  # noqa: E402

KW = {"omo": dict(dt=0.02, max_steps=40), "bob": dict(dt=0.01, max_steps=40), "qq-su": dict(dt=0.004, max_steps=40),
      "qcp-su": dict(dt=0.002, max_steps=40), "qbb": dict(dt=0.01, max_steps=40),
      "pend": dict(dt=0.02, max_steps=40, init_state=np.array([0.1, 0.2]))}
SPLITS = (7, 1, 30, 12)
ELEMENTWISE = {  # feature function -> (kind name, fp64 definition)
    F.identity_feat: ("identity", lambda x: x), F.sign_feat: ("sign", np.sign), F.abs_feat: ("abs", np.abs),
    F.squared_feat: ("squared", lambda x: x ** 2), F.cubic_feat: ("cubic", lambda x: x ** 3),
    F.sig_feat: ("sig", lambda x: 1.0 / (1.0 + np.exp(-x))), F.bell_feat: ("bell", lambda x: np.exp(-x ** 2 / 2)),
    F.sin_feat: ("sin", np.sin), F.cos_feat: ("cos", np.cos), F.sinsin_feat: ("sinsin", lambda x: np.sin(x) ** 2),
    F.sincos_feat: ("sincos", lambda x: np.sin(x) * np.cos(x))}
ALL_ELEMENTWISE = list(ELEMENTWISE)

CASES = [  # family, stack, visible rows, weight scale
    ("qq-su", (F.identity_feat, F.sin_feat, F.cos_feat), None, 4.0),
    ("qq-su", (F.const_feat, F.ATan2Feat(0, 1), F.identity_feat), [0, 1, 4, 5], 3.0),
    ("bob", (F.identity_feat, F.sign_feat, F.abs_feat, F.squared_feat, F.cubic_feat), None, 20.0),
    ("qbb", (F.identity_feat, F.sig_feat, F.bell_feat, F.MultFeat((0, 1, 2))), None, 5.0),
    ("pend", (F.sinsin_feat, F.sincos_feat, F.const_feat), None, 10.0),
    ("omo", (F.identity_feat,), None, 100.0),
    ("qcp-su", tuple(ALL_ELEMENTWISE), None, 3.0),
]


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def dev(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda()


def make_policy(vs, name, stack, idx, scale, seed):
    """LinearPolicy on the (partial) observation of family `name`, weights seeded normal times `scale`"""
    O, A = vs.env_dims(name)["O"], vs.env_dims(name)["A"]
    n_vis = len(idx) if idx is not None else O
    pol = LinearPolicy(EnvSpec(BoxSpace(-np.ones(n_vis), np.ones(n_vis)), BoxSpace(-np.ones(A), np.ones(A))),
                       F.FeatureStack(*stack))
    g = torch.Generator().manual_seed(seed)
    pol.param_values = scale * torch.randn(pol.param_values.shape, generator=g)
    return pol


def terms_fp64(stack, x):
    """the features of the definition, fp64, in stack order: [..., num_feat]"""
    cols = []
    for f in stack:
        if f is F.const_feat:
            cols.append(np.ones(x.shape[:-1] + (1,)))
        elif isinstance(f, F.MultFeat):
            cols.append(np.prod(x[..., f.idcs], axis=-1, keepdims=True))
        elif isinstance(f, F.ATan2Feat):
            cols.append(np.arctan2(x[..., f.idcs[0]], x[..., f.idcs[1]])[..., None])
        else:
            cols.append(ELEMENTWISE[f][1](x))
    return np.concatenate(cols, axis=-1)


def action_error(pol, idx, obs, act):
    """max over steps, envs and action dimensions of |act - ref| / (1 + sum_k |w_k phi_k|), ref in fp64 on the recorded obs"""
    x = obs.astype(np.float64)
    x = x[..., idx] if idx is not None else x
    phi = terms_fp64(pol.features.feat_fcns, x)
    w = pol.net.weight.detach().cpu().numpy().astype(np.float64)  # [A][F]
    ref = phi @ w.T
    scale = 1.0 + np.abs(phi) @ np.abs(w).T
    return float((np.abs(act.astype(np.float64) - ref) / scale).max()), ref


def run(e, splits, **kw):
    t = 0
    for k in splits:
        e.set_traj_offset(t)
        e.step_policy(k, record=True, **kw)
        t += k
    return e.traj(t)


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_linear_kernel_against_the_definition_and_the_step_kernel(vs, case, auto_reset):
    L = vs._lib
    name, stack, idx, scale = CASES[case]
    n, T = 700, sum(SPLITS)
    pol = make_policy(vs, name, stack, idx, scale, seed=case)
    spec = linear_kernel_spec(pol)
    assert spec is not None
    per_env = case % 2 == 0
    envs = []
    for _ in range(2):
        e = vs.VecSimEnv(name, n, **KW[name])
        if per_env:
            e.set_params(np.tile(vs.nominal_params(name), (n, 1)))
        e.set_auto_reset(auto_reset, seed=31)
        e.reset(seed=5 + case)
        envs.append(e)
    fused, ref = envs
    fused.set_policy_linear(obs_idx=idx, **spec)
    fused.set_policy_shape("256")  # (no meaning for a linear policy: ignored)
    fused.set_record_mode(2)
    fused.set_traj_capacity(T)
    tr = run(fused, SPLITS)
    # (1) the policy: recorded action against the definition on the recorded observation
    err, want = action_error(pol, idx, tr["obs"], tr["act"])
    clipped = np.abs(tr["act_app"] - tr["act"]) > 0  # (the weights are scaled so that the actions reach and leave the action box)
    print(f"{name} {[getattr(f, '__name__', type(f).__name__) for f in stack]} rows {idx} auto_reset {auto_reset}: "
          f"max |act - ref| / (1 + sum |w phi|) = {err:.2e}; |act| up to {np.abs(want).max():.1f}, {clipped.mean():.0%} clipped")
    assert np.isfinite(tr["act"]).all()
    assert err <= 1e-5
    # (2) the step: vs_step with the recorded actions from the same initial state, bit for bit
    alive = np.ones(n, dtype=bool)
    for t in range(T):
        assert np.array_equal(ref.get(L.VS_OBS)[alive], tr["obs"][t][alive]), (name, t)
        assert np.array_equal(ref.get(L.VS_STATE)[alive], tr["state"][t][alive]), (name, t)
        ref.step(dev(tr["act"][t]))
        assert np.array_equal(ref.get(L.VS_REW)[alive], tr["rew"][t][alive]), (name, t)
        assert np.array_equal(ref.get(L.VS_DONE).astype(bool)[alive], tr["done"][t].astype(bool)[alive]), (name, t)
        if not auto_reset:
            alive &= ~tr["done"][t].astype(bool)
    for which in (L.VS_STATE, L.VS_HIDDEN, L.VS_STEPCOUNT, L.VS_RETURNS):
        assert np.array_equal(ref.get(which)[alive], fused.get(which)[alive]), (name, which)
    assert tr["done"].any() and fused.error_count() == 0
    if auto_reset:
        for x, y in zip(fused.episode_stats(), ref.episode_stats()):
            assert np.array_equal(x, y)
    for e in envs:
        e.close()


@pytest.mark.parametrize("rec_mode", [1, 2])
def test_launch_cuts_do_not_show(vs, rec_mode):
    L = vs._lib
    name, stack, idx, scale = CASES[1]
    n, T = 700, sum(SPLITS)
    spec = linear_kernel_spec(make_policy(vs, name, stack, idx, scale, seed=11))
    out = []
    for splits in ((T,), SPLITS):
        e = vs.VecSimEnv(name, n, **KW[name])
        e.set_auto_reset(True, seed=3)
        e.reset(seed=8)
        e.set_policy_linear(obs_idx=idx, noise_std=0.2, **{k: v for k, v in spec.items() if k != "noise_std"})
        e.set_record_mode(rec_mode)
        e.set_traj_capacity(T)
        tr = run(e, splits, noise_seed=5)
        bufs = [e.get(w) for w in (L.VS_STATE, L.VS_OBS, L.VS_REW, L.VS_DONE, L.VS_STEPCOUNT, L.VS_RETURNS, L.VS_FAILED)]
        out.append((tr, bufs + list(e.episode_stats())))
        e.close()
    (tr_a, buf_a), (tr_b, buf_b) = out
    assert set(tr_a) == set(tr_b) and ("state" in tr_a) == (rec_mode == 2)
    for k in tr_a:
        assert np.array_equal(tr_a[k], tr_b[k]), k
    for x, y in zip(buf_a, buf_b):
        assert np.array_equal(x, y)
    # records off: the same final buffers
    e = vs.VecSimEnv(name, n, **KW[name])
    e.set_auto_reset(True, seed=3)
    e.reset(seed=8)
    e.set_policy_linear(obs_idx=idx, noise_std=0.2, **{k: v for k, v in spec.items() if k != "noise_std"})
    for k in SPLITS:
        e.step_policy(k, record=False, noise_seed=5)
    for x, y in zip([e.get(w) for w in (L.VS_STATE, L.VS_OBS, L.VS_REW, L.VS_DONE, L.VS_STEPCOUNT, L.VS_RETURNS, L.VS_FAILED)], buf_a):
        assert np.array_equal(x, y)
    e.close()


def test_exploration_noise(vs):
    name, n, T = "qbb", 4096, 24
    stack = (F.identity_feat, F.sin_feat, F.MultFeat((0, 1)))
    pol = make_policy(vs, name, stack, None, 1.0, seed=3)
    spec = linear_kernel_spec(NormalActNoiseExplStrat(pol, std_init=[0.3, 0.05]))
    std = np.array([0.3, 0.05], dtype=np.float32)
    np.testing.assert_allclose(spec["noise_std"], std)
    out = []
    for splits in ((24,), (5, 19)):
        e = vs.VecSimEnv(name, n, **KW[name])
        e.set_auto_reset(True, seed=2)
        e.reset(seed=3)
        e.set_policy_linear(**spec)
        e.set_traj_capacity(T)
        out.append(run(e, splits, noise_seed=77))
        e.close()
    a, b = out
    for key in a:
        assert np.array_equal(a[key], b[key]), key  # the noise is keyed by (env, episode, step), not by the launch
    _, mean = action_error(pol, None, a["obs"], a["act"])
    z = (a["act"] - mean) / std
    lag1 = (z[1:] * z[:-1]).mean()
    print(f"noise: mean {z.mean():.4f} std {z.std():.4f} lag-1 {lag1:.4f} cross {(z[..., 0] * z[..., 1]).mean():.4f}")
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and abs((z[..., 0] * z[..., 1]).mean()) < 0.01
    assert abs(lag1) < 0.01
    assert abs((z ** 3).mean()) < 0.03 and abs((z ** 4).mean() - 3.0) < 0.1
    c = vs.VecSimEnv(name, n, **KW[name])
    c.set_auto_reset(True, seed=2)
    c.reset(seed=3)
    c.set_policy_linear(**spec)
    c.set_traj_capacity(T)
    c.step_policy(T, record=True, noise_seed=78)
    assert not np.array_equal(c.traj(T)["act"], a["act"])  # another seed, another draw
    c.close()


@pytest.mark.parametrize("where", ["device", "host"])
def test_population_with_an_inert_group(vs, where):
    L = vs._lib
    name, n, T = "qq-su", 320, 45
    stack = (F.identity_feat, F.sin_feat, F.cos_feat, F.const_feat, F.MultFeat((0, 3)))
    pols = [make_policy(vs, name, stack, None, 4.0, seed=20 + s) for s in range(3)]
    specs = [linear_kernel_spec(p) for p in pols]
    sets = torch.stack([sp["params"] for sp in specs])
    groups = np.array([0, 1, 2, -1, 0])
    lane_set = np.repeat(groups, 64).astype(np.int32)
    inert = lane_set < 0

    def handle(s):
        e = vs.VecSimEnv(name, n, **KW[name])
        e.reset(seed=6)
        e.set_policy_linear(**specs[s])
        e.set_record_mode(2)
        e.set_traj_capacity(T)
        return e

    pop = handle(0)
    tr_before = run(pop, (T,))  # fills every lane's record rows
    pop.reset(seed=6)
    pop.set_policy_population(sets.cuda() if where == "device" else sets.numpy(), lane_set)
    st0 = pop.get(L.VS_STATE).copy()
    tr = run(pop, (20, 25))
    length, done_last = pop.rollout_lengths(n, T)
    length = length.cpu().numpy()
    assert (length[inert] == 0).all() and (length[~inert] > 0).all() and not done_last.cpu().numpy()[inert].any()
    assert np.array_equal(pop.get(L.VS_STATE)[inert], st0[inert])  # not stepped
    for k in tr:  # an inert lane's record rows keep what was there
        assert np.array_equal(tr[k][:, inert], tr_before[k][:, inert]), k
    for s in range(3):
        single = handle(s)
        tr_s = run(single, (20, 25))
        lanes = np.flatnonzero(lane_set == s)
        for k in tr:
            assert np.array_equal(tr[k][:, lanes], tr_s[k][:, lanes]), (s, k)
        len_s, _ = single.rollout_lengths(n, T)
        assert np.array_equal(length[lanes], len_s.cpu().numpy()[lanes])
        for which in (L.VS_STATE, L.VS_OBS, L.VS_RETURNS):
            assert np.array_equal(pop.get(which)[lanes], single.get(which)[lanes])
        if s == 1:  # the sets really differ
            assert not np.array_equal(tr["act"][:, lane_set == 0], tr_s["act"][:, lane_set == 0])
        single.close()
    # a population runs with records on and auto-reset off
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        pop.step_policy(4, record=False)
    pop.set_auto_reset(True, seed=1)
    with pytest.raises(RuntimeError, match=r"\(-3\).*-1 lanes"):
        pop.step_policy(4, record=True)
    with pytest.raises(vs.ValueErr):
        pop.set_policy_population(sets[:, :-1], lane_set)  # parameter count
    # setting a linear policy drops the population: auto-reset runs again and the inert lanes step
    pop.set_policy_linear(**specs[0])
    pop.set_traj_offset(0)
    pop.step_policy(4, record=True)
    assert not np.array_equal(pop.get(L.VS_STATE)[inert], st0[inert])
    pop.close()


def desc_of(L, terms, n_obs=0, obs_idx=(), noise=(0.0, 0.0)):
    d = L.LinDesc()
    d.n_terms = len(terms)
    for k, (kind, idcs) in enumerate(terms):
        d.terms[k].kind, d.terms[k].n_idx = kind, len(idcs)
        for r, x in enumerate(idcs):
            d.terms[k].idx[r] = x
    d.n_obs = n_obs
    for k, x in enumerate(obs_idx):
        d.obs_idx[k] = x
    d.noise_std[0], d.noise_std[1] = noise
    return d


def test_argument_errors_leave_the_previous_policy_working(vs):
    L = vs._lib
    lib = L.load()
    e = vs.VecSimEnv("qq-su", 128, **KW["qq-su"])
    e.reset(seed=1)
    with pytest.raises(RuntimeError):
        e.step_policy(1)  # no policy yet
    w = np.linspace(-1, 1, 12).astype(np.float32)
    e.set_policy_linear(w, ["identity", "sin"])
    e.set_traj_capacity(8)
    e.step_policy(4, record=True)
    first = e.traj(4)["act"]

    def call(desc, n_params, params=None):
        p = np.zeros(max(n_params, 1), dtype=np.float32) if params is None else params
        return lib.vs_set_policy_linear(e._h, C.byref(desc), p.ctypes.data_as(C.c_void_p), n_params)

    ID, SIN, CONST, MULT, ATAN2 = L.VS_FEAT_IDENTITY, L.VS_FEAT_SIN, L.VS_FEAT_CONST, L.VS_FEAT_MULT, L.VS_FEAT_ATAN2
    refused = [
        (desc_of(L, [(ID, ()), (SIN, ()), (ID, ())]), 18),            # an elementwise kind twice
        (desc_of(L, [(ID, ()), (MULT, (0, 6))]), 7),                  # an index outside the (six) visible rows
        (desc_of(L, [(ID, ()), (ATAN2, (0, 2))], 2, (0, 1)), 3),      # ... outside the two rows of a partial observation
        (desc_of(L, [(ID, ())], 2, (0, 6)), 2),                       # an observation row the env does not have
        (desc_of(L, [(ID, ()), (SIN, ())]), 11),                      # n_params != A F
        (desc_of(L, [(ID, ()), (99, ())]), 12),                       # an unknown kind
        (desc_of(L, [(ID, ()), (MULT, (0,))]), 7),                    # a product of one row
        (desc_of(L, [(ID, ())], noise=(-1.0, 0.0)), 6),               # a negative noise std
        (desc_of(L, [(ID, ())] + [(MULT, (0, 1))] * 40), 46),         # more product terms than the kernel keeps
    ]
    for d, npar in refused:
        assert call(d, npar) == L.VS_ERR_ARG, (d.n_terms, npar)
    full = desc_of(L, [(k, ()) for k in range(11)] + [(CONST, ())] + [(MULT, (0, 1))] * 39)  # 51 terms, 6 * 11 + 1 + 39 features
    full.n_terms = 52  # more terms than the descriptor holds
    assert call(full, 106) == L.VS_ERR_ARG
    full.n_terms = 0
    assert call(full, 106) == L.VS_ERR_ARG
    assert lib.vs_set_policy_linear(e._h, C.byref(desc_of(L, [(ID, ())])), None, 6) == L.VS_ERR_ARG  # no parameter vector
    with pytest.raises(vs.ValueErr):
        e.set_policy_linear(w, ["identity", "tanh"])
    with pytest.raises(vs.ValueErr):
        e.set_policy_linear(w[:11], ["identity", "sin"])
    # the refused calls left the policy in place: the same actions from the same state
    e.reset(seed=1)
    e.set_traj_offset(0)
    e.step_policy(4, record=True)
    assert np.array_equal(e.traj(4)["act"], first)
    # a wrapper pipeline on the handle: refused with a state error, at the setter and at the step
    e.set_act_pipeline(delay=1)
    assert call(desc_of(L, [(ID, ())]), 6) == L.VS_ERR_STATE
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        e.step_policy(1)
    e.set_act_pipeline(delay=0)
    e.step_policy(1)
    # one in-kernel policy at a time, in both directions; NULL removes it
    e.set_policy_fnn(np.zeros(6 * 8 + 8 + 8 + 1), [8], "tanh")
    e.step_policy(2)
    e.set_policy_linear(w, ["identity", "sin"])
    e.reset(seed=1)
    e.set_traj_offset(0)
    e.step_policy(4, record=True)
    assert np.array_equal(e.traj(4)["act"], first)
    e.set_policy_linear(None, None)
    with pytest.raises(RuntimeError):
        e.step_policy(1)
    e.close()
    d = vs.VecSimEnv("bob-d", 64, dt=0.01, max_steps=10)
    with pytest.raises(vs.ValueErr):
        d.set_policy_linear(np.zeros(4), ["identity"])  # discrete actions
    d.close()
    # the largest stack the kernel takes: every kind on 8 rows, the constant and 39 product / angle terms = 128 features
    q = vs.VecSimEnv("qbb", 64, **KW["qbb"])
    q.reset(seed=2)
    terms = [n for n in ("identity", "sign", "abs", "squared", "cubic", "sig", "bell", "sin", "cos", "sinsin", "sincos", "const")]
    terms += [("mult", (k % 8, (k + 3) % 8)) for k in range(38)] + [("atan2", (0, 1))]
    q.set_policy_linear(0.01 * np.random.default_rng(0).normal(size=2 * 128), terms)
    q.step_policy(3)
    assert q.error_count() == 0
    q.close()


@pytest.mark.parametrize("envname", ["qq-su", "bob"])
def test_sampler_takes_the_fused_linear_path(vs, envname, monkeypatch):
    cls = {"qq-su": vs.QQubeSwingUpSim, "bob": vs.BallOnBeamSim}[envname]
    env = cls(dt=KW[envname]["dt"], max_steps=40)
    stack = {"qq-su": (F.identity_feat, F.sin_feat, F.cos_feat, F.ATan2Feat(0, 1)),
             "bob": (F.const_feat, F.identity_feat, F.cubic_feat, F.MultFeat((0, 2)))}[envname]
    policy = LinearPolicy(env.spec, F.FeatureStack(*stack))
    g = torch.Generator().manual_seed(0)
    policy.param_values = {"qq-su": 3.0, "bob": 10.0}[envname] * torch.randn(policy.param_values.shape, generator=g)
    assert linear_kernel_spec(policy) is not None
    calls = []
    orig = vs.VecSimEnv.set_policy_linear
    monkeypatch.setattr(vs.VecSimEnv, "set_policy_linear", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    fused = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=256, seed=4)
    ros_f = fused.sample()
    assert calls  # the fused path
    calls.clear()
    loop = vs.ParallelRolloutSampler(env, policy, 1, min_rollouts=256, seed=4, fuse_policy=False)
    ros_l = loop.sample()
    assert not calls  # fuse_policy=False keeps the policy in torch
    assert len(ros_f) == len(ros_l) == 256
    policy.to("cpu")
    worst = 0.0
    for rf, rl in zip(ros_f, ros_l):
        assert np.array_equal(rf.states[0], rl.states[0]) and 1 <= len(rf) <= 40
        err, _ = action_error(policy, None, np.asarray(rf.observations[:-1], dtype=np.float32), rf.actions)
        worst = max(worst, err)
        assert rf.states.shape == (len(rf) + 1, env.state_space.flat_dim) and rf.actions_applied.shape == rf.actions.shape
        k = min(5, len(rf), len(rl))  # the first steps agree with the torch-in-the-loop path (before rounding differences grow)
        np.testing.assert_allclose(rf.observations[:k], rl.observations[:k], rtol=2e-4, atol=2e-5)
        err_l, _ = action_error(policy, None, np.asarray(rl.observations[:k], dtype=np.float32), np.asarray(rl.actions[:k]))
        assert err_l <= 1e-5
    print(f"{envname}: sampler, max |act - ref| / (1 + sum |w phi|) = {worst:.2e}")
    assert worst <= 1e-5
    # the packed form takes the same path
    (pk,) = fused.sample_packed()
    assert calls and int(pk.lengths.shape[0]) == 256
    # rollout() on a single env object: the torch path
    ro = vs.rollout(env, policy, eval=True, seed=3)
    err, _ = action_error(policy, None, np.asarray(ro.observations[:-1], dtype=np.float32), np.asarray(ro.actions))
    assert 1 <= len(ro) <= 40 and err <= 1e-5
    fused.close()
    loop.close()


def test_parameter_exploring_sampler_with_linear_policies(vs, monkeypatch):
    env = vs.QQubeSwingUpSim(dt=0.004, max_steps=40)
    stack = (F.identity_feat, F.sin_feat, F.cos_feat)

    def make():
        p = LinearPolicy(env.spec, F.FeatureStack(*stack))
        p.param_values = torch.zeros_like(p.param_values)
        return p

    policy = make()
    P, R = 4, 10
    params = 3.0 * torch.randn(P, policy.param_values.numel(), generator=torch.Generator().manual_seed(5))
    np.random.seed(1)
    inits = [env.init_space.sample_uniform() for _ in range(R)]
    calls = []
    orig = vs.VecSimEnv.set_policy_population
    monkeypatch.setattr(vs.VecSimEnv, "set_policy_population", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    smp = vs.ParameterExploringSampler(env, policy, R, 1, seed=2)
    assert smp._fused()
    res = smp.sample(params, init_states=inits)
    assert calls and len(res) == P and all(s.num_rollouts == R for s in res)
    calls.clear()
    smp2 = vs.ParameterExploringSampler(env, policy, R, 1, seed=2)
    ret = smp2.sample_returns(params, init_states=inits)
    assert calls and tuple(ret.returns.shape) == (P, R)
    calls.clear()
    # sample() and sample_returns(): the same rollouts
    want = np.array([[ro.undiscounted_return() for ro in s.rollouts] for s in res])
    np.testing.assert_allclose(ret.returns.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    assert np.array_equal(ret.lengths.cpu().numpy(), np.array([[len(ro) for ro in s.rollouts] for s in res]))
    # ... and those of four single-policy runs on the same Philox keys
    for s in range(P):
        pol_s = make()
        pol_s.param_values = params[s]
        ros = vs.ParallelRolloutSampler(env, pol_s, 1, min_rollouts=R, seed=2).sample(init_states=inits)
        assert not calls
        for a, b in zip(res[s].rollouts, ros):
            assert np.array_equal(a.observations, b.observations) and np.array_equal(a.actions, b.actions)
            assert np.array_equal(a.rewards, b.rewards) and np.array_equal(a.states, b.states)
    assert not ParameterExploringSampler_fused(vs, env, policy, fuse_policy=False)
    assert torch.equal(policy.param_values, torch.zeros_like(policy.param_values))
    smp.close()
    smp2.close()


def ParameterExploringSampler_fused(vs, env, policy, **kw):
    s = vs.ParameterExploringSampler(env, policy, 2, 1, **kw)
    try:
        return s._fused()
    finally:
        s.close()
