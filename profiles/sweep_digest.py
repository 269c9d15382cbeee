"""SHA-256 of every output of the reverse-mode kernels on small fixed cases, to compare two builds of libvecsim bit for bit:

    VS_LIB_PATH=OLD/libvecsim.so python profiles/sweep_digest.py old.txt
    VS_LIB_PATH=NEW/libvecsim.so python profiles/sweep_digest.py new.txt   &&   diff old.txt new.txt

One line per (case, set of cotangents given): the digest over the raw bytes of d_act, d_init (+ d_hid, d_hid0 for the recurrent sweep;
for vs_fnn_param_grad d_params stored and accumulated), all lanes of the leading dimension included.  n = 65 lanes (the leading dimension is the library's: one full
wave, a partial one and lanes >= n, whose length is 0), t_steps = 33 (the done-bit word boundary is real), capacity 64 rows.  The
rollouts are recorded by the policy of the case from sampled initial states; then done bits are OR-ed into the recorded words so
that every case has the three kinds of lane whatever the family's own failures give: lane 3k ends at row 1 + k % 30 (first word), lane
3k + 1 at row 32 (second word), lane 3k + 2 keeps its own bits (it runs to the end unless it failed); and every lane gets a stale bit
at row 40, behind t_steps.  The script checks the three groups with vs_rollout_lengths and fails if one is empty.
Cotangents: all given, all NULL, and each one NULL in turn.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simurlacra_amd as vs  # noqa: E402
from simurlacra_amd import _lib as L  # noqa: E402

N, T, CAP = 65, 33, 64
DT = {"pend": 0.01, "qq-su": 0.004, "qcp-su": 0.002, "qbb": 0.01}
LINES = []


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def vec(*modules):
    return torch.nn.utils.parameters_to_vector([p for m in modules for p in m.parameters()]).detach().to(torch.float32)


def recorded(name, set_policy):
    """a handle whose rows 0 .. T - 1 hold closed-loop rollouts of the three kinds of length"""
    e = vs.VecSimEnv(name, N, dt=DT[name], max_steps=4000)
    assert e.ld > N and e.ld % 64 == 0, e.ld  # lanes >= n exist: their length is 0
    e.set_auto_reset(False)
    e.reset(seed=1)
    e.set_record_mode(2)
    e.set_traj_capacity(CAP)
    set_policy(e)
    e.step_policy(T, record=True)
    e.sync()
    words = e.traj_planes()[1]
    lane = torch.arange(e.ld, device=words.device)
    first = torch.where(lane % 3 == 0, torch.ones_like(lane) << (1 + (lane // 3) % 30), torch.zeros_like(lane))
    second = torch.where(lane % 3 == 1, torch.ones_like(lane), torch.zeros_like(lane)) | (1 << (40 - 32))
    words[0] |= first.to(words.dtype)
    words[1] |= second.to(words.dtype)
    torch.cuda.synchronize()
    length, done_last = e.rollout_lengths(N, T)
    groups = [int((length <= 32).sum()), int(((length == T) & done_last).sum()), int(((length == T) & ~done_last).sum())]
    assert min(groups) > 0, f"{name}: a length group is empty: {groups}"
    assert e.error_count() == 0, name
    return e, groups


def cotangents(e, names, extra=()):
    S, A, O, H = (e.dims[k] for k in "SAOH")
    g = torch.Generator(device="cpu").manual_seed(7)
    shapes = {"g_rew": (T, e.ld), "g_obs": (T + 1, O, e.ld), "g_act": (T, A, e.ld), "g_state_last": (S + H, e.ld), **dict(extra)}
    return {k: torch.randn(*shapes[k], generator=g).cuda() for k in names}


def combos(names):
    yield "all given", set(names)
    yield "all NULL", set()
    for k in names:
        yield f"{k} NULL", set(names) - {k}


def run(case, e, groups, sweep, names, extra=()):
    full = cotangents(e, names, extra)
    kept = None
    for label, given in combos(names):
        out = sweep(T, **{k: (full[k] if k in given else None) for k in names})
        e.sync()
        if label == "all given":
            kept = out[0]
        LINES.append(f"{case:28s} {label:18s} lengths {groups} {digest(*out)}")
    return kept


def plain(name):
    A, O = vs.env_dims(name)["A"], vs.env_dims(name)["O"]
    torch.manual_seed(1)
    W = 0.1 * torch.randn(A, O)
    e, groups = recorded(name, lambda e: e.set_policy_linear(W.reshape(-1), ["identity"]))
    run(f"vjp {name}", e, groups, e.rollout_vjp, ("g_rew", "g_obs", "g_state_last"))
    e.close()


def linear():
    name, idx, terms = "pend", (2, 0), ["identity", "sin", "const", ("mult", (0, 1)), ("atan2", (0, 1))]
    A = vs.env_dims(name)["A"]
    torch.manual_seed(2)
    W = 0.1 * torch.randn(A, 2 + 2 + 1 + 1 + 1)
    e, groups = recorded(name, lambda e: e.set_policy_linear(W.reshape(-1), terms, obs_idx=idx))
    run("vjp_policy pend view", e, groups, e.rollout_vjp_policy, ("g_rew", "g_obs", "g_act", "g_state_last"))
    e.close()


def fnn(name, hidden, feat, idx):
    A, O = vs.env_dims(name)["A"], vs.env_dims(name)["O"]
    n_in = (O if idx is None else len(idx)) + (1 if feat else 0)
    torch.manual_seed(3)
    sizes = [n_in] + list(hidden)
    layers = [torch.nn.Linear(a, b) for a, b in zip(sizes[:-1], sizes[1:])] + [torch.nn.Linear(sizes[-1], A)]
    with torch.no_grad():
        layers[-1].weight.mul_(0.2)
    e, groups = recorded(name, lambda e: e.set_policy_fnn(vec(*layers), list(hidden), hidden_nonlin="tanh", feat=feat, obs_idx=idx))
    case = f"fnn {name} {'x'.join(map(str, hidden))}{' feat' if feat else ''}{' view' if idx else ''}"
    abar = run("vjp_" + case, e, groups, e.rollout_vjp_fnn, ("g_rew", "g_obs", "g_act", "g_state_last"))
    stored = e.fnn_param_grad(T, abar)
    acc = torch.linspace(-1.0, 1.0, stored.numel(), device=stored.device)
    e.fnn_param_grad(T, abar, out=acc, accumulate=True)
    e.sync()
    LINES.append(f"{'param_grad ' + case:28s} {'stored, accumulated':18s} lengths {groups} {digest(stored, acc)}")
    e.close()


def rnn(name, cell, n_layers, H):
    A, O = vs.env_dims(name)["A"], vs.env_dims(name)["O"]
    torch.manual_seed(4)
    cls = {"tanh": torch.nn.RNN, "gru": torch.nn.GRU, "lstm": torch.nn.LSTM}[cell]
    net, out = cls(O, H, n_layers), torch.nn.Linear(H, A)
    with torch.no_grad():
        out.weight.mul_(0.2)
    Hs = n_layers * H * (2 if cell == "lstm" else 1)

    def set_policy(e):
        e.set_policy_rnn(vec(net, out), cell=cell, n_layers=n_layers, hidden_size=H)
        e.set_policy_hidden_record(Hs)

    e, groups = recorded(name, set_policy)
    run(f"vjp_rnn {name} {cell} {n_layers}x{H}", e, groups, e.rollout_vjp_rnn, ("g_rew", "g_obs", "g_act", "g_state_last", "g_hid_last"),
        extra=(("g_hid_last", (Hs, e.ld)),))
    e.close()


def main():
    for name in ("pend", "qq-su", "qcp-su", "qbb"):
        plain(name)
    linear()
    for idx in (None, (0, 1, 3, 2, 5)):
        fnn("qq-su", [64], False, idx)
        fnn("qq-su", [64, 64], True, idx)
    for cell in ("tanh", "gru", "lstm"):
        for n_layers in (1, 2):
            for H in (33, 64):
                rnn("qq-su", cell, n_layers, H)
    text = "\n".join(LINES)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
