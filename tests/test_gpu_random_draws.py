"""
Every device random draw held to its distribution and to independence.

All draws of the library come from one Philox generator keyed by (seed, global env index, purpose, episode or step).  The reference
draws from NumPy's global generator, so the distribution is the specification: each purpose's draws are mapped back to standard
variates by the fp64 inverse maps of random_draw_checks.py (written from oracle.cpu_ref, not from the kernels) and held to the four
non-asymptotic bounds there -- marginal, correlation, joint_cells, frequency -- per dimension, between the dimensions of one draw,
between lanes (i against i + 1, i + 64, i + 256), between steps or episodes, between seeds (the high word included), between
shards, and between the purposes under one seed value.  No threshold is tuned against the device; no stream layout or counter
arithmetic of the kernels is encoded.  test_random_draw_checks_host.py shows on the host that an ideal generator passes at these
sample sizes and that the planted faults fail.

Every seed argument is 7 unless the seed itself is under test.  The last test prints the worst ratio per (purpose, check) with -s
(profiles/random_draw_digest.txt) and asserts checks * ALPHA <= 1e-6.
"""
import numpy as np
import pytest

import random_draw_checks as rc
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ENVS = ["omo", "bob", "qq-su", "qcp-su", "qbb", "qq-st", "qcp-st", "pend", "bob-d"]
KW = {"omo": dict(dt=0.02, max_steps=300), "bob": dict(dt=0.01, max_steps=500), "qq-su": dict(dt=0.004, max_steps=4000),
      "qcp-su": dict(dt=0.002, max_steps=8000), "qbb": dict(dt=0.01, max_steps=500),
      "qq-st": dict(dt=0.01, max_steps=500), "qcp-st": dict(dt=0.01, max_steps=300),
      "pend": dict(dt=0.02, max_steps=400, init_state=np.array([0.1, 0.2])), "bob-d": dict(dt=0.01, max_steps=500)}
N, T, EPISODES, REDRAWS, SHARDS = 16384, 64, 9, 8, 4  # (the sizes test_random_draw_checks_host.py runs the ideal generator at)
SEED = 7
OTHER_SEEDS = (8, 7 + 2 ** 32)  # the high word is half of the key
BOOK = rc.Book()
SPECS = rc.PARAM_SPECS


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def lane_params(name, n=N):
    """+-15 % around nominal, per lane (float32): the oscillator's action bound and the init bounds of ball-on-beam and the ball
    balancer then differ from lane to lane"""
    ref = cpu_ref.make_ref(name, **KW[name])
    p = ref.nominal_params(n)
    return ref, (p * np.random.default_rng(ENVS.index(name)).uniform(0.85, 1.15, p.shape)).astype(np.float32)


def handle(vs, name, params, offset=0, seed=SEED, **kw):
    e = vs.VecSimEnv(name, params.shape[0], **dict(KW[name], **kw))
    e.set_index_offset(offset)
    e.set_params(params)
    e.set_auto_reset(True, seed=seed)  # every lane then acts at every step
    e.reset(seed=seed)
    return e


# ------------------------------------------------------------------------------------------------------------------- actions
def recorded_actions(vs, name, params, variant="k_rollout", normed=False, seed=SEED, seek=None, offset=0):
    e = handle(vs, name, params, offset)
    e.set_act_norm(normed)
    e.set_rollout_variant(variant)
    if seek is not None:
        e.seek_random(seek)
    e.step_random(T, seed=seed, record=True)
    act = e.traj(T)["act"]
    assert e.error_count() == 0
    e.close()
    return act


@pytest.mark.parametrize("normed", [False, True])
@pytest.mark.parametrize("name", ENVS)
def test_action_draws(vs, name, normed):
    """RNG_ACT: 64 recorded steps of the plain kernel under per-lane parameters; the automatic choice of kernel and a shard
    reproduce them bit for bit"""
    ref, params = lane_params(name)
    act = recorded_actions(vs, name, params, normed=normed)
    rc.battery(BOOK, "actions", rc.action_variates(ref, act, params.astype(np.float64), normed), step_lags=(1, 4 // ref.A),
               what=f"{name} normed={normed}")
    if not normed:
        assert np.array_equal(recorded_actions(vs, name, params, variant=None), act)
        assert np.array_equal(recorded_actions(vs, name, params[N // 2:], offset=N // 2), act[:, N // 2:])


@pytest.mark.parametrize("name", ["omo", "qbb"])
def test_action_draws_across_the_32_bit_boundary_of_the_step_counter(vs, name):
    """after seek_random(2^34 - 8) the 64 steps take the stream's counter across 2^32 blocks, for A = 1 and for A = 2.  A stream that
    dropped the high word of the step counter would repeat the run from step 0 from row 8 on: rows 8 .. are held against rows 0 .. of
    that run, beside the aligned rows."""
    ref, params = lane_params(name)
    act = recorded_actions(vs, name, params, seek=2 ** 34 - 8)
    vs_ = rc.action_variates(ref, act, params.astype(np.float64))
    rc.battery(BOOK, "actions", vs_, step_lags=(1, 4 // ref.A), what=f"{name} after the seek")
    base = rc.action_variates(ref, recorded_actions(vs, name, params), params.astype(np.float64))
    rc.hold_against(BOOK, "actions", vs_, base, f"{name} after the seek x from step 0")
    rc.hold_shifted(BOOK, "actions", vs_, base, 8, f"{name} rows 8 .. after the seek x rows 0 .. from step 0")


@pytest.mark.parametrize("name", ["omo", "qbb"])
def test_action_draws_between_seeds_and_shards(vs, name):
    ref, params = lane_params(name)
    p64 = params.astype(np.float64)
    base = rc.action_variates(ref, recorded_actions(vs, name, params), p64)
    for s in OTHER_SEEDS:
        other = rc.action_variates(ref, recorded_actions(vs, name, params, seed=s), p64)
        rc.hold_against(BOOK, "actions", base, other, f"{name} seed {SEED} x seed {s}")
    shard = rc.action_variates(ref, recorded_actions(vs, name, params, offset=N), p64)
    rc.hold_against(BOOK, "actions", base, shard, f"{name} lanes 0 .. n - 1 x lanes n .. 2 n - 1")


# --------------------------------------------------------------------------------------------------------------- init states
def init_rows(vs, name, params, seed=SEED, offset=0):
    """[EPISODES, n, S]: row 0 the draw of reset(seed), rows 1 .. 8 the draws of the auto-resets of episodes 1 .. 8 (max_steps = 1:
    every step ends an episode; record mode 2 keeps the state each step started from)"""
    e = handle(vs, name, params, offset, seed=seed, max_steps=1)
    s0 = e.get(vs._lib.VS_STATE)
    e.set_record_mode(2)
    e.step_random(EPISODES, seed=seed, record=True)
    tr = e.traj(EPISODES)
    assert tr["done"].all() and np.array_equal(tr["state"][0], s0)
    e.close()
    return tr["state"]


@pytest.mark.parametrize("name", [n for n in ENVS if n != "pend"])
def test_init_state_draws(vs, name):
    """RNG_INIT: reset(seed) and the auto-resets of eight episodes under per-lane parameters.  init_variates first asserts that
    every row lies inside its lane's init space, which is what licenses reading it as a draw."""
    ref, params = lane_params(name)
    st = init_rows(vs, name, params)
    vs_ = rc.init_variates(ref, st, params.astype(np.float64))
    rc.battery(BOOK, "init", vs_, what=name)
    if name in ("bob", "bob-d"):  # the side bit, an atom beside continuous variates, from episode to episode by itself
        rc.hold_lagged(BOOK, "init", vs_[:1], 0, 1, f"{name} side bit, row t x t + 1")
    assert np.array_equal(init_rows(vs, name, params[N // 2:], offset=N // 2), st[:, N // 2:])


def test_singular_init_space_draws_nothing(vs):
    ref, params = lane_params("pend")
    st = init_rows(vs, "pend", params)
    assert rc.init_variates(ref, st, params.astype(np.float64)) == []


@pytest.mark.parametrize("name", ["bob", "qbb"])
def test_init_state_draws_between_seeds_and_shards(vs, name):
    ref, params = lane_params(name)
    p64 = params.astype(np.float64)
    base = rc.init_variates(ref, init_rows(vs, name, params), p64)
    pool = [v for v in base if v.probs is None]
    for s in OTHER_SEEDS:
        other = rc.init_variates(ref, init_rows(vs, name, params, seed=s), p64)
        rc.hold_against(BOOK, "init", base, other, f"{name} seed {SEED} x seed {s}")
        pool += [v for v in other if v.probs is None]
    shard = rc.init_variates(ref, init_rows(vs, name, params, offset=N), p64)
    rc.hold_against(BOOK, "init", base, shard, f"{name} lanes 0 .. n - 1 x lanes n .. 2 n - 1")
    pool += [v for v in shard if v.probs is None]
    u = np.concatenate([v.u.ravel() for v in pool])  # every continuous init variate of the four handles: U(0, 1), independent
    assert u.size >= 2 ** 20
    BOOK.hold("init", "marginal", rc.marginal(u, max(v.q for v in pool)), f"{name} pooled over dimensions, seeds and shards")


# --------------------------------------------------------------------------------------------------------- domain parameters
PARAM_ENV = "qq-su"  # 11 parameters; SPECS: [uniform, normal, normal, uniform, clipped normal, Bernoulli, rounded normal, normal, normal]


def sampled_params(vs, n=N, seed=SEED, offset=0):
    e = vs.VecSimEnv(PARAM_ENV, n, **KW[PARAM_ENV])
    e.set_index_offset(offset)
    e.sample_params(SPECS, seed=seed)
    P = e.get(vs._lib.VS_PARAMS)
    e.close()
    return P


def redrawn_params(vs):
    """[REDRAWS, n, P]: the live randomizer's redraws at the auto-resets of eight episodes of one step"""
    ref = cpu_ref.make_ref(PARAM_ENV, **KW[PARAM_ENV])
    e = handle(vs, PARAM_ENV, ref.nominal_params(N).astype(np.float32), max_steps=1)
    e.set_randomizer(SPECS)
    rows = []
    for _ in range(REDRAWS):
        e.step_random(1, seed=SEED)
        rows.append(e.get(vs._lib.VS_PARAMS))
    e.close()
    return np.stack(rows)


def test_domain_parameter_draws(vs):
    """RNG_PARAM: sample_params on four shards of 16 384 lanes (65 536 lanes, what the 10 % fault needs) and the live redraw.  A
    normal takes two words of a block of four: the second normal and the last but one straddle block boundaries."""
    names = list(cpu_ref.ENV_REFS[PARAM_ENV].param_names)
    nominal = cpu_ref.ENV_REFS[PARAM_ENV].nominal_params(1)[0].astype(np.float32)
    P = np.stack([sampled_params(vs, offset=k * N) for k in range(SHARDS)])
    R = redrawn_params(vs)
    touched = [names.index(s[0]) for s in SPECS]
    for X in (P, R):
        rest = [j for j in range(len(names)) if j not in touched]
        assert (X[..., rest] == nominal[rest]).all()
    first = rc.param_variates(SPECS, names, P)
    live = rc.param_variates(SPECS, names, R)
    rc.battery(BOOK, "params", first, what="sample_params")
    rc.battery(BOOK, "params", live, what="live redraw")
    bern = [v for v, s in zip(live, SPECS) if s[1] == "bernoulli"]  # the Bernoulli redraw from episode to episode by itself
    rc.hold_lagged(BOOK, "params", bern, 0, 1, "Bernoulli, live redraw t x t + 1")
    rc.hold_against(BOOK, "params", [v.rows(slice(0, 1)) for v in first], [v.rows(slice(0, 1)) for v in live],
                    "sample_params x first live redraw")
    pool = [v for v in first + live if v.probs is None]
    u = np.concatenate([v.u.ravel() for v in pool])
    assert u.size >= 2 ** 20
    BOOK.hold("params", "marginal", rc.marginal(u, max(v.q for v in pool)), "all continuous parameters")
    # seeds, and a shard bit for bit
    for s in OTHER_SEEDS:
        other = rc.param_variates(SPECS, names, sampled_params(vs, seed=s)[None])
        rc.hold_against(BOOK, "params", [v.rows(slice(0, 1)) for v in first], other, f"seed {SEED} x seed {s}")
    assert np.array_equal(sampled_params(vs, n=N // 2, offset=N // 2), P[0, N // 2:])


def test_parameter_buffer_random_selection(vs):
    """selection='random': the set a lane takes at an auto-reset is uniform over the buffer, independent across lanes and episodes"""
    B = 6
    ref = cpu_ref.make_ref("omo", **KW["omo"])
    e = handle(vs, "omo", ref.nominal_params(N).astype(np.float32), max_steps=1)
    e.set_param_buffer([dict(mass=1.0 + 0.125 * k) for k in range(B)], selection="random")
    rows = []
    for _ in range(REDRAWS):
        e.step_random(1, seed=SEED)
        rows.append(e.get(vs._lib.VS_PARAMS)[:, 0])
    e.close()
    k = (np.stack(rows).astype(np.float64) - 1.0) / 0.125
    assert np.array_equal(k, np.rint(k))
    rc.battery(BOOK, "params", [rc.set_index_variate(k.astype(np.int64), B)], what="buffer set")


# --------------------------------------------------------------------------------------------------------- exploration noise
BIAS = {"qq-su": np.array([0.25], dtype=np.float32), "qbb": np.array([0.25, -0.5], dtype=np.float32)}
STD = {"qq-su": np.array([0.5], dtype=np.float32), "qbb": np.array([0.5, 0.25], dtype=np.float32)}


def set_constant_policy(vs, e, name, kind):
    """all-zero weights and the bias BIAS: the policy's mean is exactly BIAS, so z = (act - BIAS) / STD is exact"""
    d = vs.env_dims(name)
    O, A, b = d["O"], d["A"], BIAS[name]
    if kind in ("64", "256", "mfma"):
        H = 16
        e.set_policy_fnn(np.concatenate([np.zeros(H * O + H + A * H, dtype=np.float32), b]), [H], noise_std=STD[name])
        e.set_policy_shape(kind)
    elif kind == "gru":
        H = 8
        e.set_policy_rnn(np.concatenate([np.zeros(3 * H * O + 3 * H * H + 6 * H + A * H, dtype=np.float32), b]), cell="gru",
                         hidden_size=H, noise_std=STD[name])
    else:  # LinearPolicy has no bias: the weight of a constant feature beside the identity term
        W = np.zeros((A, O + 1), dtype=np.float32)
        W[:, O] = b
        e.set_policy_linear(W.reshape(-1), ["identity", "const"], noise_std=STD[name])


def noise_variates(vs, name, kind, seed=SEED, offset=0, n=N):
    ref = cpu_ref.make_ref(name, **KW[name])
    e = handle(vs, name, ref.nominal_params(n).astype(np.float32), offset)
    set_constant_policy(vs, e, name, kind)
    e.set_traj_capacity(T)
    t = 0
    for k in (7, 1, 56):
        e.set_traj_offset(t)
        e.step_policy(k, record=True, noise_seed=seed)
        t += k
    act = e.traj(T)["act"]
    e.close()
    return act, [rc.normal_variate(f"z{j}", act[..., j], BIAS[name][j], STD[name][j]) for j in range(act.shape[-1])]


@pytest.mark.parametrize("name,kind", [("qbb", k) for k in ("64", "256", "mfma", "gru", "linear")]
                         + [("qq-su", k) for k in ("64", "gru", "linear")])
def test_exploration_noise_draws(vs, name, kind):
    """RNG_POLICY_NOISE in each of the three rollout bodies that draw it (feed-forward in its three shapes, recurrent, linear), with
    a std per action dimension and 64 steps in launches of 7 + 1 + 56"""
    act, zs = noise_variates(vs, name, kind)
    rc.battery(BOOK, "noise", zs, what=f"{name} {kind}")
    if kind == "64":
        for s in OTHER_SEEDS:
            rc.hold_against(BOOK, "noise", zs, noise_variates(vs, name, kind, seed=s)[1], f"{name} seed {SEED} x seed {s}")
        rc.hold_against(BOOK, "noise", zs, noise_variates(vs, name, kind, offset=N)[1], f"{name} lanes 0 .. n - 1 x n .. 2 n - 1")
        assert np.array_equal(noise_variates(vs, name, kind, offset=N // 2, n=N // 2)[0], act[:, N // 2:])
    else:  # one stream whatever the policy: the other bodies repeat the feed-forward body's draws
        assert np.array_equal(noise_variates(vs, name, "64")[0], act)


# ------------------------------------------------------------------------------------------------------------ across purposes
def test_purposes_are_independent_under_one_seed_value(vs):
    """dimension 0 of the action draw, the init draw, the first parameter draw, the exploration noise and the observation noise of
    the same lanes at step / episode 0, every seed argument 7: every pair passes correlation and joint_cells"""
    L = vs._lib
    name = PARAM_ENV
    ref = cpu_ref.make_ref(name, **KW[name])
    nominal = ref.nominal_params(N)
    names = list(ref.param_names)
    draws = {}
    act = recorded_actions(vs, name, nominal.astype(np.float32))
    draws["action"] = rc.action_variates(ref, act[:1], nominal)[0]
    draws["init"] = rc.init_variates(ref, init_rows(vs, name, nominal.astype(np.float32))[:1], nominal)[0]
    draws["param"] = rc.param_variates(SPECS[:1], names, sampled_params(vs)[None])[0]
    draws["noise"] = rc.normal_variate("z0", noise_variates(vs, name, "64")[0][:1, :, 0], BIAS[name][0], STD[name][0])
    # the observation noise, recovered as test_observation_noise_statistics_and_keys does (6 dims, 12 steps)
    scale = np.array([1.0, 2.0, 0.5, 1.0, 0.05, 0.04])
    shift = np.array([0.0, -1.0, 0.25, 0.0, 0.1, 0.0])
    std = np.array([0.1, 0.2, 0.05, 0.3, 1.5, 0.01])
    e = vs.VecSimEnv(name, N, **KW[name])
    e.set_obs_pipeline(scale, shift, std, seed=SEED)
    e.reset(seed=SEED)
    zero = torch.zeros(N, 1, device="cuda")
    zs = []
    for t in range(13):
        inner = ref.observe(e.get(L.VS_STATE).astype(np.float64))
        zs.append((e.get(L.VS_OBS).astype(np.float64) - (inner * scale + shift)) / std)
        if t < 12:
            e.step(zero)
    e.close()
    z = np.stack(zs)  # [13, n, 6]
    assert abs(z.std() - 1.0) < 0.01
    # (q: the observation of dimension 0 is below 1 in size and its noise has std 0.1)
    draws["obs noise"] = rc.Var("obs z0", rc.Phi(z[:1, :, 0]), q=float(np.spacing(np.float32(1.0))) / std[0])
    keys = list(draws)
    for k, a in enumerate(keys):
        for b in keys[k + 1:]:
            rc.hold_pair(BOOK, "purposes", draws[a], draws[b], draws[a].u, draws[b].u, f"{a} x {b}")


def test_zz_digest_and_budget(vs):
    """the digest of the whole module (run alone it has nothing to print, and says so by failing)"""
    assert BOOK.n > 0 and {p for p, _ in BOOK.worst} == {"actions", "init", "params", "noise", "purposes"}, "run with the whole module"
    print("\n" + rc.digest_header(vs._lib.load().vs_version()))
    print(BOOK.report())
    BOOK.assert_budget()
