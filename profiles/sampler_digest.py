"""SHA-256 of everything the rollout samplers return on small seeded cases, to compare two versions of the host package bit for bit
on ONE built library:

    VS_LIB_PATH=simurlacra_amd/csrc/libvecsim.so python profiles/sampler_digest.py --package-root OLD_TREE old.txt
    VS_LIB_PATH=simurlacra_amd/csrc/libvecsim.so python profiles/sampler_digest.py --package-root . new.txt  &&  diff old.txt new.txt

--package-root: the directory that holds the simurlacra_amd package to import (default: this checkout).

One line per case and call: `rollouts`, the digest over every array of every StepSequence of sample() in rollout order
(observations, actions, rewards, states, actions_applied, th_ddot, hidden_states, init_state, the done flags and rollout_info), or
`packed`, the digest over every tensor field of every PackedRollouts of sample_packed() / sample_returns(); then `calls`, the number
and the digest of the library calls the case made, in order, by name and plain number arguments (pointers left out; so are the
queries that neither launch, copy nor change a handle: vs_get, vs_ld, vs_env_dims, vs_param_name, vs_nominal_params,
vs_traj_layout, vs_record_mode, vs_last_error).

Every path of ParallelRolloutSampler._run_batch once, on qq-su and bob: 65 rollouts (one past a wave) of at most 40 steps, 16 steps
per launch (two full launches and a partial one; bob's rollouts also end early), 48 lanes per batch for the split.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

N, T, CHUNK = 65, 40, 16
DT = {"qq-su": 0.004, "bob": 0.01}
QUERIES = {"vs_get", "vs_ld", "vs_env_dims", "vs_param_name", "vs_nominal_params", "vs_traj_layout", "vs_record_mode",
           "vs_last_error"}
LINES, CALLS = [], []


class LoggedLibrary:
    """the loaded library with every vs_* call noted in CALLS"""

    def __init__(self, lib):
        self._real = lib

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("vs_") or name in QUERIES:
            return fn

        def logged(*args):
            CALLS.append((name,) + tuple(a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool)))
            return fn(*args)
        return logged


def sha(parts):
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, torch.Tensor):
            p = p.detach().cpu().numpy()
        if isinstance(p, np.ndarray):
            h.update(str((p.dtype, p.shape)).encode())
            h.update(np.ascontiguousarray(p).tobytes())
        else:
            h.update(repr(p).encode())
    return h.hexdigest()


def rollout_parts(ros):
    for ro in ros:
        for k in ("observations", "actions", "rewards", "states", "actions_applied", "th_ddot", "hidden_states", "init_state"):
            yield k
            yield getattr(ro, k, None)
        yield ro.done
        yield sorted((k, sorted(v.items()) if isinstance(v, dict) else v) for k, v in ro.rollout_info.items())


def packed_parts(packs):
    for p in packs:
        for k in sorted(p.__dict__):
            yield k
            yield p.__dict__[k]


def digest_of(out):
    """(what was returned, its digest) of sample() / sample_packed() of either sampler and of sample_returns()"""
    if hasattr(out, "packed"):  # PopulationReturns
        return f"packed   {len(out.packed):4d}", sha(list(packed_parts(out.packed)) + [out.parameters, out.returns, out.lengths])
    if hasattr(out, "parameters"):  # ParameterSamplingResult
        flat = [ro for s in out for ro in s.rollouts]
        return f"rollouts {len(flat):4d}", sha(list(rollout_parts(flat)) + [out.parameters])
    if out and hasattr(out[0], "rows"):  # [PackedRollouts]
        return f"packed   {len(out):4d}", sha(packed_parts(out))
    return f"rollouts {len(out):4d}", sha(rollout_parts(out))


def case(label, make, call="sample", **kw):
    """one call of a fresh sampler make() with kw: a line for what it returned, a line for the library calls it made"""
    np.random.seed(11)
    torch.manual_seed(12)
    del CALLS[:]
    smp = make()
    kind, digest = digest_of(getattr(smp, call)(**kw))
    torch.cuda.synchronize()
    smp.close()
    LINES.append(f"{label:44s} {call:14s} {kind} {digest}")
    LINES.append(f"{label:44s} {call:14s} calls    {len(CALLS):4d} {sha(CALLS)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))

    import simurlacra_amd as vs
    from simurlacra_amd import _lib as L
    from simurlacra_amd import features as F

    assert os.path.abspath(vs.__file__).startswith(os.path.abspath(args.package_root)), vs.__file__
    L._lib = LoggedLibrary(L.load())
    PRS, PES = vs.ParallelRolloutSampler, vs.ParameterExploringSampler

    def env_of(name):
        return vs.ENV_CLASSES[name](dt=DT[name], max_steps=T)

    def net(cls, env, *a, **k):
        torch.manual_seed(5)
        return cls(env.spec, *a, **k)

    def prs(env, pol, **k):
        return lambda: PRS(env, pol, 1, **{**dict(min_rollouts=N, seed=3, chunk=CHUNK), **k})

    for name in ("qq-su", "bob"):
        np.random.seed(9)
        env = env_of(name)
        A = env.act_space.flat_dim
        dummy = vs.DummyPolicy(env.spec)
        fnn = net(vs.FNNPolicy, env, [16, 16], torch.tanh)
        gru = net(vs.GRUPolicy, env, 16, 1)
        lin = net(vs.LinearPolicy, env, F.FeatureStack(F.identity_feat, F.sin_feat))
        noisy = vs.NormalActNoiseExplStrat(net(vs.FNNPolicy, env, [16], torch.tanh), std_init=0.3)
        rng = np.random.default_rng(7)
        play = vs.PlaybackPolicy(env.spec, [rng.normal(size=(t, A)).astype(np.float32) for t in (40, 17, 25)])
        inits = [env.init_space.sample_uniform() for _ in range(3)]
        dps = [{"gravity_const": 9.0 + 0.5 * i} for i in range(2)]
        both = ("sample", "sample_packed")
        for pol_name, pol, kw in (("dummy", dummy, {}), ("fnn fused", fnn, {}), ("fnn + noise fused", noisy, {}), ("gru fused", gru, {}),
                                  ("linear fused", lin, {}), ("playback fused", play, {}),
                                  ("playback torch", play, dict(fuse_policy=False)), ("fnn torch", fnn, dict(fuse_policy=False)),
                                  ("gru torch", gru, dict(fuse_policy=False)),
                                  ("fnn graph", fnn, dict(fuse_policy=False, graph_policy=True)),
                                  ("gru graph", gru, dict(fuse_policy=False, graph_policy=True)),
                                  ("dummy lean records", dummy, dict(full_records=False)),
                                  ("gru fused lean records", gru, dict(full_records=False)),
                                  ("dummy owned arrays", dummy, dict(owned_arrays=True)),
                                  ("dummy split", dummy, dict(batch_lanes=48)), ("fnn fused split", fnn, dict(batch_lanes=48)),
                                  ("gru torch split", gru, dict(fuse_policy=False, batch_lanes=48))):
            for call in both:
                case(f"{name} {pol_name}", prs(env, pol, **kw), call)
        for call in both:
            case(f"{name} dummy inits x params", prs(env, dummy, min_rollouts=7), call, init_states=inits, domain_params=dps)
            case(f"{name} fnn fused inits", prs(env, fnn), call, init_states=inits)
            case(f"{name} fnn torch params split", prs(env, fnn, fuse_policy=False, batch_lanes=48), call, domain_params=dps)
        case(f"{name} dummy min_steps", prs(env, dummy, min_rollouts=None, min_steps=1500, batch_lanes=48))
        live = vs.DomainRandWrapperLive(env_of(name), vs.create_default_randomizer(env))
        ring = vs.DomainRandWrapperBuffer(env_of(name), vs.create_default_randomizer(env))
        np.random.seed(13)
        ring.fill_buffer(5)
        for call in both:
            case(f"{name} dummy live randomizer", prs(live, dummy), call)
            case(f"{name} fnn fused ring buffer", prs(ring, fnn), call)
        chain = vs.ObsPartialWrapper(vs.ObsNormWrapper(vs.ActNormWrapper(vs.ActDelayWrapper(env_of(name), delay=2))),
                                     mask=[0] * (env.obs_space.flat_dim - 1) + [1])
        partial = vs.ObsPartialWrapper(env_of(name), mask=[0] * (env.obs_space.flat_dim - 1) + [1])
        for call in both:
            case(f"{name} dummy wrapper chain", prs(chain, vs.DummyPolicy(chain.spec)), call)
            case(f"{name} fnn torch wrapper chain", prs(chain, net(vs.FNNPolicy, chain, [16], torch.tanh)), call)
            case(f"{name} fnn fused partial obs", prs(partial, net(vs.FNNPolicy, partial, [16], torch.tanh)), call)
        # populations: 5 sets x (2 domains x 3 init states), fused in one batch, in batches of whole sets, and the host loop
        for pol_name, pol in (("fnn", fnn), ("gru", gru), ("linear", lin)):
            torch.manual_seed(6)
            p0 = pol.param_values.detach().clone()
            sets = torch.stack([p0 + 0.1 * torch.randn_like(p0) for _ in range(5)])
            for tag, kw in (("", {}), (" split", dict(batch_lanes=128)), (" host loop", dict(fuse_policy=False))):
                mk = lambda kw=kw, pol=pol: PES(live, pol, 3, 2, seed=3, chunk=CHUNK, **kw)  # (two draws of the randomizer)
                case(f"{name} population {pol_name}{tag}", mk, "sample", param_sets=sets)
                if "loop" not in tag:
                    case(f"{name} population {pol_name}{tag}", mk, "sample_returns", param_sets=sets, gamma=0.99)
            pol.param_values = p0
    text = "\n".join(LINES)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
