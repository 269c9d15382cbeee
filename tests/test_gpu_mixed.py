"""
The mixed-family launch (vs_mixed_*, MixedVecSimEnv; k_rollout_mixed / k_step_mixed) against the same members run as stand-alone
VecSimEnv handles: same index offsets, seeds and settings, stepped by vs_step_random / vs_step, pinned to "k_rollout" (the body
the mixed launch runs).  The comparison is np.array_equal on every per-env buffer, on episode_stats() and on every field of
traj() where the launch records.  One step per family also goes against the fp64 oracle, at the state tolerance of
test_gpu_parity.py.

Shapes: max_steps = 40 and 50 steps cut into launches of 7 + 1 + 30 + 12, so every lane ends its episode inside a launch.
  group A  omo 1, bob 257, qq-su 64, qcp-su 300, qbb 255      five members (MAX_SEG), a one-lane and a one-workgroup segment
  group B  qq-st 256, qcp-st 63, pend 65, bob-d 513           four members; with A all nine cases of MIXED_DISPATCH
  group C  qq-su 100, qq-su 100                                one family twice: own dt, own per-lane parameters (+- 5 %)
  group D  qbb 130                                             a single member
  group R  bob 257, qq-su 64, qbb 130                          the group of the refusal tests
Member sizes 1, 63, 64, 65, 255, 256, 257, 513: below, on and above the 64-lane wave and the 256-lane workgroup.

Instantiations launched (asserted per case by `instantiation`, from the settings that select them):
  k_rollout_mixed<AR, REC, DRK>  <0,0,0> <0,1,0> <0,2,0> <1,0,0> <1,1,0> <1,2,0> <1,0,1> <1,1,1> <1,2,1>
  k_step_mixed<AR, DRK>          <0,0> <1,0> <1,1>
"""
import ctypes as C

import numpy as np
import pytest

from oracle import cpu_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_parity as par  # noqa: E402  (KW, the state tolerance and its constants)

MAX_STEPS, T, CUTS = 40, 50, (7, 1, 30, 12)
SEED_RESET, SEED_ACT, SEED_AR = 5, 9, 21
GROUPS = {"A": [("omo", 1), ("bob", 257), ("qq-su", 64), ("qcp-su", 300), ("qbb", 255)],
          "B": [("qq-st", 256), ("qcp-st", 63), ("pend", 65), ("bob-d", 513)],
          "C": [("qq-su", 100), ("qq-su", 100)],
          "D": [("qbb", 130)],
          "R": [("bob", 257), ("qq-su", 64), ("qbb", 130)]}
DT_C = (0.004, 0.006)  # group C: the two members differ in dt
# the members that redraw domain parameters at a reset inside the launch (the DRK instantiations): member index -> what it carries.
# No draw and no buffer set equals the nominal value, so a redrawn lane differs from its initial parameters.
RANDOMIZER = {"A": (2, [("mass_pend_pole", "uniform", 0.028, 0.002, 0.0, 1.0), ("length_pend_pole", "normal", 0.14, 0.004, 0.131, 0.16)]),
              "B": (2, [("pole_mass", "uniform", 1.2, 0.1, 0.0, 10.0), ("pole_length", "normal", 1.1, 0.02, 1.02, 1.2)])}
BUFFER = {"A": (4, [dict(ball_mass=0.0035, ball_damping=0.04), dict(ball_mass=0.004, gravity_const=9.7), dict(ball_mass=0.0045)]),
          "B": (1, [dict(cart_mass=0.5), dict(cart_mass=0.62, pole_damping=0.003), dict(cart_mass=0.66)])}
BUFFERS = ("STATE", "HIDDEN", "OBS", "REW", "DONE", "FAILED", "STEPCOUNT", "RETURNS", "PARAMS", "ERRFLAG")


@pytest.fixture(scope="module")
def vs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simurlacra_amd

    return simurlacra_amd


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).cuda()


# ------------------------------------------------------------------------------------------------------------ building
def configure(vs, group, ar, rec, drk=False, pin="k_rollout", bookkeeping=False):
    """The handles of a group before the group is formed; members and stand-alone copies are made by this one function.
    rec: 0 (no records) | 1 | 2.  bookkeeping (case 2): member 1 has 13 random steps behind it, member 2 resets with another seed,
    member 3 records from row 5 of 55 behind a sentinel."""
    L = vs._lib
    out = []
    for q, (name, n) in enumerate(GROUPS[group]):
        kw = dict(par.KW[name], max_steps=MAX_STEPS)
        if group == "C":
            kw["dt"] = DT_C[q]
        e = vs.VecSimEnv(name, n, **kw)
        if group == "C":
            p = np.tile(vs.nominal_params(name), (n, 1))
            e.set_params((p * (1 + 0.05 * np.random.default_rng(100 + q).uniform(-1, 1, p.shape))).astype(np.float32))
        case = dict(kw=kw, ar=bool(ar), redraw=None, t0=0, p0=e.get(L.VS_PARAMS))
        if drk and RANDOMIZER[group][0] == q:
            e.set_randomizer(RANDOMIZER[group][1])
            case["redraw"] = "randomizer"
        if drk and BUFFER[group][0] == q:
            e.set_param_buffer(BUFFER[group][1], "cyclic")
            case["redraw"] = "buffer"
        e.set_auto_reset(ar, seed=SEED_AR + (100 if bookkeeping and q == 2 else 0))
        e.set_record_mode(rec or 1)
        if rec:
            e.set_traj_capacity(T)
        if bookkeeping and q == 3 and rec:
            case["t0"] = 5
            e.set_traj_capacity(T + 5)
            planes, words = e.traj_planes()
            for p, _ in planes:
                p[:5] = 7.0
            words[0] = 0b10101  # the done bits of rows 0, 2 and 4
            torch.cuda.synchronize()
        e.set_rollout_variant(pin)
        e.reset(seed=SEED_RESET)
        if bookkeeping and q == 1:
            e.step_random(13, seed=SEED_ACT)  # on its own, before the group is formed: its action stream stands at step 13
            case["pre"] = 13
        e._case = case
        out.append(e)
    return out


def form(vs, handles, mixed):
    """the group (mixed) or the same index offsets on stand-alone handles; then the start states, drawn by global lane index"""
    mx = vs.MixedVecSimEnv(handles) if mixed else None
    off = 0
    for e in handles:
        if not mixed:
            e.set_index_offset(off)
        off += e.n_envs
        if "pre" not in e._case:
            e.reset(seed=SEED_RESET)
    return mx


def instantiation(handles, record):
    """<AR, REC, DRK> of the k_rollout_mixed a launch of these members runs (launch_rollout_mixed; k_step_mixed: <AR, DRK>), from the
    settings that select it"""
    ar = {e._case["ar"] for e in handles}
    modes = {e.record_mode for e in handles}
    assert len(ar) == 1 and len(modes) == 1
    ar = ar.pop()
    return ar, (modes.pop() if record else 0), ar and any(e._case["redraw"] is not None for e in handles)


def launches(target, handles, cuts, rec, t_start=0):
    """target: the MixedVecSimEnv (one launch per cut) or None (one vs_step_random per handle and cut)"""
    t = t_start
    for k in cuts:
        for e in handles:
            if rec:
                e.set_traj_offset(e._case["t0"] + t)
        if target is not None:
            target.step_random(k, seed=SEED_ACT, record=bool(rec))
        else:
            for e in handles:
                e.step_random(k, seed=SEED_ACT, record=bool(rec))
        t += k


def snapshot(vs, e, rec):
    L = vs._lib
    s = {k: e.get(getattr(L, "VS_" + k)) for k in BUFFERS}
    s["es_count"], s["es_retsum"], s["es_lensum"] = e.episode_stats()
    if rec:
        s.update({"traj_" + k: v for k, v in e.traj(e._traj_cap).items()})
    return s


def assert_same(got, exp, label):
    assert got.keys() == exp.keys(), label
    for k in exp:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (label, k)
        assert np.array_equal(got[k], exp[k]), (label, k, int((got[k] != exp[k]).sum()))


def close_all(*groups):
    for g in groups:
        for e in g:
            e.close()


_SOLO = {}


def solo_reference(vs, group, ar, rec, drk=False, pin="k_rollout", bookkeeping=False, cuts=CUTS):
    """The stand-alone run of a configuration, computed once: per member its snapshot after the launches.  What every case asserts
    of the reference itself -- the kernel it ran, that every lane ended an episode, that the redraws happened -- is asserted here."""
    key = (group, ar, rec, drk, pin, bookkeeping, cuts)
    if key in _SOLO:
        return _SOLO[key]
    solo = configure(vs, group, ar, rec, drk, pin, bookkeeping)
    form(vs, solo, mixed=False)
    if pin is not None:
        assert all(e.rollout_variant() == pin for e in solo)
    launches(None, solo, cuts, rec)
    snaps = [snapshot(vs, e, rec) for e in solo]
    for e, s in zip(solo, snaps):
        assert s["ERRFLAG"].sum() == 0
        if ar:
            assert s["es_count"].min() >= 1 and (s["STEPCOUNT"] < MAX_STEPS).all(), e.name  # every lane ended an episode and restarted
        else:
            assert s["DONE"].all() and (s["es_count"] == 1).all(), e.name  # every lane ended its episode and froze
        if rec:
            assert s["traj_done"][e._case["t0"]:].any(axis=0).all(), e.name
        changed = (s["PARAMS"] != e._case["p0"]).any(axis=1)
        assert changed.all() if (ar and e._case["redraw"]) else not changed.any(), (e.name, e._case["redraw"])
    close_all(solo)
    _SOLO[key] = snaps
    return snaps


def mixed_run(vs, group, ar, rec, drk=False, bookkeeping=False, cuts=CUTS, expect=None):
    members = configure(vs, group, ar, rec, drk, bookkeeping=bookkeeping)
    mx = form(vs, members, mixed=True)
    if expect is not None:
        assert instantiation(members, rec) == expect
    launches(mx, members, cuts, rec)
    snaps = [snapshot(vs, e, rec) for e in members]
    mx.close()
    close_all(members)
    return snaps


# --------------------------------------------------------------------------------------------- 1. every instantiation
@pytest.mark.parametrize("rec", [0, 1, 2])
@pytest.mark.parametrize("ar,drk", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("group", ["A", "B"])
def test_every_rollout_instantiation_equals_standalone_handles(vs, group, ar, drk, rec):
    """k_rollout_mixed<AR, REC, DRK>, all nine, on the five- and the four-member group: all nine families.  Under DRK one member
    carries a live randomizer, one a cyclic parameter buffer and the others nothing to redraw."""
    ref = solo_reference(vs, group, ar, rec, drk)
    got = mixed_run(vs, group, ar, rec, drk, expect=(ar, rec, drk))
    for q, (g, r) in enumerate(zip(got, ref)):
        assert_same(g, r, (group, q, GROUPS[group][q]))


@pytest.mark.parametrize("group,pin", [("C", None), ("D", "k_rollout")])
def test_one_family_twice_and_single_member(vs, group, pin):
    """Group C: two segments of one family with their own Task (dt) and Dev (per-lane parameters); its stand-alone handles choose
    their kernel themselves.  Group D: a group of one."""
    ref = solo_reference(vs, group, True, 2, pin=pin)
    if group == "C":
        probe = configure(vs, group, True, 2, pin=pin)
        assert all(e.rollout_variant() != "k_rollout" for e in probe)  # the automatic choice is another kernel at this size
        close_all(probe)
        assert not np.array_equal(ref[0]["STATE"], ref[1]["STATE"]) and not np.array_equal(ref[0]["PARAMS"], ref[1]["PARAMS"])
    got = mixed_run(vs, group, True, 2, expect=(True, 2, False))
    for q, (g, r) in enumerate(zip(got, ref)):
        assert_same(g, r, (group, q))


# ------------------------------------------------------------------------------------------ 2. per-segment bookkeeping
def test_every_segment_keeps_its_own_epoch_reset_seed_and_record_offset(vs):
    """Seg::epoch0, ::reset_seed and Dev::traj_t0 differ between the members: member 1 is 13 steps into its action stream, member
    2 resets with another seed, member 3 records from row 5 of 55.  Rows 0 .. 4 of member 3 keep the sentinel, bits included."""
    ref = solo_reference(vs, "A", True, 2, bookkeeping=True)
    got = mixed_run(vs, "A", True, 2, bookkeeping=True, expect=(True, 2, False))
    for q, (g, r) in enumerate(zip(got, ref)):
        assert_same(g, r, ("A", q))
    plain = solo_reference(vs, "A", True, 2)  # the same group with nothing special: the three settings do change the run
    for q in (1, 2):
        assert not np.array_equal(ref[q]["STATE"], plain[q]["STATE"]), q
    for snaps in (ref, got):
        tr = {k: v for k, v in snaps[3].items() if k.startswith("traj_")}
        assert tr["traj_obs"].shape[0] == T + 5
        for k, v in tr.items():
            if k == "traj_done":
                assert np.array_equal(v[:5], np.tile(np.array([1, 0, 1, 0, 1], dtype=v.dtype)[:, None], (1, v.shape[1])))
            else:
                assert (v[:5] == 7.0).all(), k
        assert np.array_equal(tr["traj_obs"][5:], plain[3]["traj_obs"])  # member 3 itself runs as ever, five rows further down


# ------------------------------------------------------------------------------------ 3. action layouts in vs_mixed_step
def act_scale(name, kw):
    ref = cpu_ref.make_ref(name, **kw)
    return ref, np.abs(ref.bounds(ref.nominal_params(1))[3][0])


def laid_out(base, kind, rng):
    """base [N, A] float32 as a device tensor of the given layout (what VecSimEnv.step and MixedVecSimEnv.step both accept)"""
    n, a = base.shape
    if kind == "1d" and a != 1:
        kind = "slice"
    if kind == "rows":
        return dev(base)
    if kind == "transposed":
        return dev(base.T.copy()).t()  # [N, A] view of an [A, N] tensor: env stride 1, dim stride N
    if kind == "1d":
        return dev(base[:, 0])
    wide = rng.uniform(-1e3, 1e3, (n, a + 3)).astype(np.float32)
    wide[:, 1:1 + a] = base
    return dev(wide)[:, 1:1 + a]  # env stride A + 3, an offset base pointer


LAYOUTS = ("rows", "transposed", "1d", "slice")


def step_group(vs, ar, drk=False):
    members, solo = configure(vs, "A", ar, 0, drk), configure(vs, "A", ar, 0, drk)
    mx = form(vs, members, mixed=True)
    form(vs, solo, mixed=False)
    return members, solo, mx


@pytest.mark.parametrize("ar,drk", [(False, False), (True, False), (True, True)])
def test_action_layouts_in_mixed_step(vs, ar, drk):
    """k_step_mixed<AR, DRK>, all three: every call passes a row-major, a transposed, a 1-D and a column-slice tensor, and the
    layouts move on by one member per step, so the two-dimensional action of qbb comes transposed (dim stride N), as a slice and
    row-major.  Under auto-reset the lanes stand at steps 38 and 37: they time out and restart in steps 2 and 3."""
    L = vs._lib
    members, solo, mx = step_group(vs, ar, drk)
    rng = np.random.default_rng(17)
    if ar:
        for e in members + solo:
            e.put(L.VS_STEPCOUNT, np.where(np.arange(e.n_envs) % 2 == 0, 38, 37).astype(np.int32))
    assert instantiation(members, 0) == (ar, 0, drk)  # k_step_mixed<ar, drk>
    for t in range(3):
        acts, kinds = [], []
        for q, e in enumerate(members):
            scale = act_scale(e.name, e._case["kw"])[1]
            base = (rng.uniform(-1.3, 1.3, (e.n_envs, e.dims["A"])) * scale).astype(np.float32)
            kinds.append(LAYOUTS[(q + t + 1) % 4])
            acts.append(laid_out(base, kinds[-1], rng))
        assert set(kinds) == set(LAYOUTS)
        if t < 2:
            assert not acts[4].is_contiguous()  # qbb: transposed, then a slice
        mx.step(acts)
        for e, a in zip(solo, acts):
            e.step(a)
        for q, (a, b) in enumerate(zip(members, solo)):
            sb = snapshot(vs, b, 0)
            assert_same(snapshot(vs, a, 0), sb, (t, q, kinds[q]))
            if ar and t >= 1:
                timed_out = (np.arange(b.n_envs) % 2 == 0) if t == 1 else (np.arange(b.n_envs) % 2 == 1)
                assert (sb["es_count"][timed_out] >= 1).all() and (sb["STEPCOUNT"][timed_out] == 0).all()
    for b in solo:
        changed = (b.get(L.VS_PARAMS) != b._case["p0"]).any(axis=1)
        assert changed.all() if b._case["redraw"] else not changed.any()
    mx.close()
    close_all(members, solo)


def test_nan_actions_flag_the_same_lanes(vs):
    """NaN in lane 0 of the first member and in the last lane of the last: VS_ERRFLAG and error_count(), member by member"""
    L = vs._lib
    members, solo, mx = step_group(vs, False)
    acts = [np.zeros((e.n_envs, e.dims["A"]), dtype=np.float32) for e in members]
    acts[0][0, 0] = np.nan
    acts[-1][-1, -1] = np.nan
    acts = [dev(a) for a in acts]
    mx.step(acts)
    for e, a in zip(solo, acts):
        e.step(a)
    for q, (a, b) in enumerate(zip(members, solo)):
        exp = np.zeros(b.n_envs, dtype=np.uint8)
        if q == 0:
            exp[0] = 1
        if q == len(solo) - 1:
            exp[-1] = 1
        assert np.array_equal(b.get(L.VS_ERRFLAG), exp) and np.array_equal(a.get(L.VS_ERRFLAG), exp), q
        assert a.error_count() == b.error_count() == int(exp.sum())
    mx.close()
    close_all(members, solo)


@pytest.mark.parametrize("group", ["A", "B"])
def test_one_mixed_step_against_the_oracle(vs, group):
    """one vs_mixed_step without auto-reset per family against oracle/cpu_ref.py (fp64) on the same fp32 inputs, at the state
    tolerance of test_gpu_parity.py: the dispatch cases compared with something that is not the same code"""
    L = vs._lib
    members = configure(vs, group, False, 0)
    mx = form(vs, members, mixed=True)
    rng = np.random.default_rng(23)
    before, acts = [], []
    for e in members:
        ref, scale = act_scale(e.name, e._case["kw"])
        before.append((ref, e.get(L.VS_STATE).astype(np.float64), e.get(L.VS_HIDDEN).astype(np.float64), e.get(L.VS_STEPCOUNT),
                       e.get(L.VS_PARAMS).astype(np.float64)))
        acts.append((rng.uniform(-1.3, 1.3, (e.n_envs, e.dims["A"])) * scale).astype(np.float32))
    assert instantiation(members, 0) == (False, 0, False)
    mx.step([dev(a) for a in acts])
    for e, (ref, s0, h0, c0, p), a in zip(members, before, acts):
        exp = ref.step(s0, h0, a.astype(np.float64), p, c0)
        par.assert_state_close(ref, e.get(L.VS_STATE), exp["state"], p)
        assert np.array_equal(e.get(L.VS_STEPCOUNT), c0 + 1) and e.error_count() == 0
    mx.close()
    close_all(members)


# ------------------------------------------------------------------------------------- 4. launch cuts and repeatability
def test_launch_cuts_and_repeated_runs_give_the_same_bits(vs):
    ref = solo_reference(vs, "A", True, 1)
    whole = mixed_run(vs, "A", True, 1, cuts=(T,), expect=(True, 1, False))
    cut = mixed_run(vs, "A", True, 1, cuts=CUTS)
    again = mixed_run(vs, "A", True, 1, cuts=CUTS)
    for q in range(len(ref)):
        assert_same(whole[q], ref[q], ("one launch", q))
        assert_same(cut[q], whole[q], ("cuts", q))
        assert_same(again[q], cut[q], ("again", q))


# ------------------------------------------------------------------------------------------------------- 5. refusals
class Refusals:
    """Group R (auto-reset on, record mode 1) with the first launch of 7 steps done.  refused() checks the code, that the message
    names the cause and that no member's buffer or record changed; finish() runs the remaining launches and holds the members to
    stand-alone handles that never saw a refused call."""

    def __init__(self, vs, first=True):
        self.vs, self.L, self.lib = vs, vs._lib, vs._lib.load()
        self.members = configure(vs, "R", True, 1)
        self.mx = form(vs, self.members, mixed=True)
        assert instantiation(self.members, 1) == (True, 1, False)
        self.t = 0
        if first:
            self.launch(CUTS[:1])

    def launch(self, cuts):
        launches(self.mx, self.members, cuts, 1, self.t)
        self.t += sum(cuts)

    def state(self):
        return [snapshot(self.vs, e, 1) for e in self.members]

    def step_random(self, k, record=1):
        return self.lib.vs_mixed_step_random(self.mx._h, SEED_ACT, k, record)

    def step(self, replace=None):
        """vs_mixed_step with zero actions; replace: {member: another address for its actions}"""
        n = len(self.members)
        self.acts = [torch.zeros(e.n_envs, e.dims["A"], device="cuda") for e in self.members]
        ptrs = [(replace or {}).get(q, a.data_ptr()) for q, a in enumerate(self.acts)]
        return self.lib.vs_mixed_step(self.mx._h, (C.c_void_p * n)(*ptrs), (C.c_int64 * n)(*[a.stride(0) for a in self.acts]),
                                      (C.c_int64 * n)(*[a.stride(1) for a in self.acts]))

    def refused(self, call, code, cause):
        before = self.state()
        rc = call()
        msg = self.lib.vs_mixed_last_error(self.mx._h).decode()
        assert rc == code, (rc, msg)
        assert cause in msg, msg
        for q, (a, b) in enumerate(zip(self.state(), before)):
            assert_same(a, b, (cause, q))

    def finish(self):
        done = 0
        rest = []
        for k in CUTS:
            if done >= self.t:
                rest.append(k)
            done += k
        assert self.t + sum(rest) == T
        self.launch(tuple(rest))
        ref = solo_reference(self.vs, "R", True, 1)
        for q, (a, b) in enumerate(zip(self.state(), ref)):
            assert_same(a, b, ("after the refusals", q))
        self.mx.close()
        close_all(self.members)


def test_create_refusals(vs):
    """vs_mixed_create: six members, members that differ in auto-reset, the same handle twice -- VS_ERR_ARG, no handle, and the
    handles serve a group afterwards as if nothing had been asked"""
    L, lib = vs._lib, vs._lib.load()
    r = Refusals(vs, first=False)
    extra = configure(vs, "R", False, 1)  # three more handles, auto-reset off
    before = r.state()

    def create(handles):
        out = C.c_void_p()
        rc = lib.vs_mixed_create((C.c_void_p * len(handles))(*[e._h for e in handles]), len(handles), C.byref(out))
        if out.value:
            lib.vs_mixed_destroy(out)
        return rc, bool(out.value), lib.vs_last_error(None).decode()

    m = r.members
    for handles, cause in ((m + extra, "1..5"), ([m[0], extra[1]], "auto-reset"), ([m[0], m[1], m[0]], "twice"), ([m[2], m[2]], "twice")):
        rc, made, msg = create(handles)
        assert rc == L.VS_ERR_ARG and not made and cause in msg, (cause, rc, made, msg)
        for q, (a, b) in enumerate(zip(r.state(), before)):
            assert_same(a, b, (cause, q))
    close_all(extra)
    r.finish()


def test_launch_refusals_leave_every_member_where_it_was(vs):
    """record modes that differ, a record that does not fit, k_steps = 0, host memory for the actions"""
    r = Refusals(vs, first=False)
    L, m = r.L, r.members
    m[1].set_record_mode(2)  # (drops member 1's record buffers: before the first recorded launch)
    m[1].set_traj_capacity(T)
    r.refused(lambda: r.step_random(7), L.VS_ERR_STATE, "record mode")
    m[1].set_record_mode(1)
    m[1].set_traj_capacity(T)
    r.launch(CUTS[:1])
    m[2].set_traj_offset(T - 6)
    r.refused(lambda: r.step_random(7), L.VS_ERR_STATE, "vs_set_traj_capacity")
    r.refused(lambda: r.step_random(0), L.VS_ERR_ARG, "k_steps must be >= 1")
    r.refused(lambda: r.step_random(-1, record=0), L.VS_ERR_ARG, "k_steps must be >= 1")
    host = np.zeros((m[2].n_envs, 2), dtype=np.float32)
    r.refused(lambda: r.step(replace={2: host.ctypes.data}), L.VS_ERR_ARG, "device memory")
    r.finish()


def test_pipeline_refusal_moves_no_random_stream(vs):
    """A wrapper pipeline on the LAST of three members: the launch is refused before the action streams of the first two move,
    so that the launches after the pipeline is removed equal those of handles that never saw the refusal."""
    r = Refusals(vs)
    L, m = r.L, r.members
    m[2].set_act_pipeline(delay=1)
    r.refused(lambda: r.step_random(1), L.VS_ERR_STATE, "pipeline")
    r.refused(lambda: r.step_random(30, record=0), L.VS_ERR_STATE, "pipeline")
    r.refused(lambda: r.step(), L.VS_ERR_STATE, "pipeline")
    m[2].set_act_pipeline(delay=0)
    m[0].set_obs_pipeline(scale=np.full(m[0].dims["O"], 2.0))
    r.refused(lambda: r.step_random(1), L.VS_ERR_STATE, "pipeline")
    m[0].set_obs_pipeline()
    r.finish()


def test_flipped_auto_reset_is_refused_by_both_launches(vs):
    """vs_set_auto_reset on one member after the group was formed: vs_mixed_step refuses as vs_mixed_step_random does, in the
    same words, instead of running everybody with the first member's setting"""
    r = Refusals(vs)
    L, m = r.L, r.members
    m[1].set_auto_reset(False, seed=SEED_AR)
    r.refused(lambda: r.step_random(1), L.VS_ERR_STATE, "vs_mixed_step_random: segments differ in auto-reset")
    r.refused(lambda: r.step(), L.VS_ERR_STATE, "vs_mixed_step: segments differ in auto-reset")
    m[1].set_auto_reset(True, seed=SEED_AR)
    r.finish()


def test_member_on_another_stream_is_refused(vs):
    """vs_set_stream on a member after the group was formed: the launch runs on one stream, and this member's own resets and
    copies would no longer be ordered with it.  Every member on one stream again: accepted."""
    r = Refusals(vs)
    L, m = r.L, r.members
    m[1].use_stream(None)  # back to its own stream
    r.refused(lambda: r.step_random(1), L.VS_ERR_STATE, "stream")
    r.refused(lambda: r.step(), L.VS_ERR_STATE, "stream")
    side = torch.cuda.Stream()
    for e in m:
        e.use_stream(side.cuda_stream)
    r.finish()
