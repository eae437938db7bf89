"""One restatement of one `DQNTrainer.optimize_device` call with any of its options on (test helper, numpy; torch only as
the container `noisy_ref.composed_state_dict` hands back), put together from the references every option already has:

  nstep_ref.compose          the minibatch the sampling launch composes from the record ring
  noisy_ref                  the noise of a draw (`layer_noise64`, rounded once to float32 like the device's vectors), the
                             float32 composition of the dense head (`compose32` through `composed_state_dict`) and the
                             sigmas' gradient (`sigma_grad32`)
  dueling_ref / gcn_ref64    forward, loss term and backward of every graph, for the three heads
  target_net_ref             the Double-DQN choice (`select`) and the Polyak step (`polyak`)
  adam_ref.step              the Adam update over the trained entries of the flat layout

Every function takes `dtype` the way gcn_ref64 does: float64 is the reference, float32 the yardstick of what fp32
arithmetic alone costs (`chain_pair` runs it forced to the fp64 run's TopK selections and Double-DQN choices).  What stays
float32 in both: the ring's records, the composed weights (the device composes them in float32, bit for bit), the Polyak
step.  Two places where a float32 helper would put a rounding into the fp64 run are taken in `dtype` instead, with the
helper's own decision: the Double-DQN value is the target's output of the column `target_net_ref.select` picks, and the
sigmas' gradient is `sigma_grad32`'s product formed in fp64.

`chain_pair` also reports, per graph, every decision of the fp64 run that sits closer to flipping than the helpers' own
threshold (`gcn_train_cases.KINK` fp32 yardsticks of its quantity): the TopK / relu / readout decisions of every forward
the graph takes part in (`gcn_train_cases.kink_violations`), the argmax the select launch or mode 1 takes
(`dueling_ref.argmax_gaps`) and the Huber branch (the distance of |td| from 1 against the yardstick of td)."""
import types

import numpy as np
import torch

import adam_ref
import dueling_ref as dref
import gcn_ref64 as ref
import gcn_train_cases as tc
import noisy_ref
import nstep_ref
import target_net_ref
from nstep_ref import Nstep

KINK = tc.KINK


# ------------------------------------------------------------------ what the restatement has to know of a network
def arch_of(net):
    """dict(levels, ratio, head, params [(name, shape, trained)] in `parameters()` order - the flat layout of the gradient
    and the Adam moments -, noisy: `noisy_layout()` or None)."""
    from meshdqn_amd.gcn_fused import _levels_of
    mods, _ = _levels_of(net)
    names = {id(m): k for k, m in net.named_modules()}
    unused = {id(p) for p in net.unused_parameters()}
    return dict(levels=[(names[id(c)], names[id(p)]) for c, p in mods], ratio=float(mods[0][1].ratio), head=net.head,
                params=[(k, tuple(p.shape), id(p) not in unused) for k, p in net.named_parameters()],
                noisy=net.noisy_layout() if getattr(net, "noisy", None) is not None else None)


def host_sd(net):
    """The network's state dict as float32 numpy arrays (a copy: what a later kernel writes does not show)."""
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def offsets(arch):
    """{name: (lo, hi, shape)} of the flat layout and its length."""
    out, off = {}, 0
    for k, shape, _ in arch["params"]:
        n = int(np.prod(shape))
        out[k] = (off, off + n, shape)
        off += n
    return out, off


def flat_of(sd, arch, dtype=np.float32):
    return np.concatenate([ref._arr(sd[k], dtype).reshape(-1) for k, _, _ in arch["params"]])


def trained_mask(arch):
    return np.concatenate([np.full(int(np.prod(shape)), used, bool) for _, shape, used in arch["params"]])


class _Holder:
    """What `noisy_ref.composed_state_dict` asks of a network, from a state dict."""

    def __init__(self, sd, layout):
        self._sd = {k: torch.from_numpy(ref._arr(v, np.float32).copy()) for k, v in sd.items()}
        self.noisy_sigma, self._layout = self._sd["noisy_sigma"], layout

    def state_dict(self):
        return self._sd

    def noisy_layout(self):
        return self._layout


def composed(sd, arch, draw, eps=None):
    """(the plain state dict the network is under draw (seed, stream, counter), {layer: (eps_in, eps_out)} float32).  No
    draw: the means.  `eps`: vectors to use in place of the draw's (e.g. the device's own)."""
    if draw is None and eps is None:
        return {k: ref._arr(v, np.float32) for k, v in sd.items() if k != "noisy_sigma"}, None
    if eps is None:
        n64 = noisy_ref.layer_noise64(int(draw[0]), int(draw[1]), int(draw[2]), arch["noisy"])
        eps = {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in n64.items()}
    csd = noisy_ref.composed_state_dict(_Holder(sd, arch["noisy"]), eps)
    return {k: v.numpy() for k, v in csd.items()}, eps


def graphs_of(mb, which, N):
    """[(x (N, F), edge_index (2, E))] of the minibatch's states (`which` = "s") or next states ("n")."""
    ptr = mb["edge_ptr_" + which]
    return [(mb["x_" + which][b].reshape(N, -1),
             np.stack([mb["esrc_" + which][ptr[b]:ptr[b + 1]], mb["edst_" + which][ptr[b]:ptr[b + 1]]]).astype(np.int64))
            for b in range(len(mb["x_" + which]))]


def forwards(sd, arch, graphs, dtype=np.float64, forced=None):
    return [dref.forward_graph(sd, arch["levels"], x, ei, arch["ratio"], arch["head"], dtype, None if forced is None else forced[b])
            for b, (x, ei) in enumerate(graphs)]


# ------------------------------------------------------------------ the learning step of a minibatch
def learning_step(sd, levels, head, runs, mode, action, reward, nonfinal, gamma, q_other, weight=None, dtype=np.float64):
    """`dueling_ref.learning_step_graph` over the graphs of a minibatch (`runs`: their forward runs in `dtype`):
    dict(steps [per graph: term, td, grads, amax], td (B,), terms (B,), loss: the terms summed in graph order)."""
    dt = np.dtype(dtype).type
    B = len(runs)
    steps = [dref.learning_step_graph(sd, levels, runs[b], head, mode, int(action[b]), reward[b], nonfinal[b], gamma, q_other[b], B,
                                      None if weight is None else float(weight[b]), dtype) for b in range(B)]
    return dict(steps=steps, td=np.array([s["td"] for s in steps], dt), terms=np.array([s["term"] for s in steps], dt),
                loss=reduce_loss(steps, range(B), dtype))


def reduce_loss(steps, keep, dtype=np.float64):
    s = np.dtype(dtype).type(0)
    for b in keep:
        s = s + steps[b]["term"]
    return s


def _sigma_grad(g_w, g_b, eps_in, eps_out, dtype):
    if np.dtype(dtype) == np.float32:
        return noisy_ref.sigma_grad32(g_w, g_b, eps_in, eps_out)
    e_in, e_out = np.asarray(eps_in, np.float64), np.asarray(eps_out, np.float64)       # (sigma_grad32's product, in fp64)
    return g_w * (e_out[:, None] * e_in[None, :]), g_b * e_out


def reduce_grad(steps, keep, arch, eps=None, dtype=np.float64):
    """({name: the graphs' gradients summed in graph order, `noisy_sigma` from the summed means' gradients}, the same
    as one flat vector in the device's layout); a parameter no graph touches is zero."""
    dt = np.dtype(dtype).type
    offs, total = offsets(arch)
    grads = {}
    for k, shape, _ in arch["params"]:
        if k == "noisy_sigma":
            continue
        s = np.zeros(shape, dt)
        for b in keep:
            g = steps[b]["grads"].get(k)
            if g is not None:
                s = s + np.asarray(g, dt).reshape(shape)
        grads[k] = s
    if arch["noisy"] is not None:
        sig = np.zeros(offs["noisy_sigma"][2], dt)
        if eps is not None:
            for name, o, i, off_w, off_b in arch["noisy"]:
                w, b_ = _sigma_grad(grads[name + ".weight"], grads[name + ".bias"], *eps[name], dtype)
                sig[off_w:off_w + o * i], sig[off_b:off_b + o] = np.asarray(w, dt).reshape(-1), np.asarray(b_, dt)
        grads["noisy_sigma"] = sig
    return grads, np.concatenate([grads[k].reshape(-1) for k, _, _ in arch["params"]]).astype(dt)


def adam_apply(p, m, v, g, hp, mask, dtype=np.float64):
    """`adam_ref.step` on the trained entries (`mask`) of the flat layout; the others keep p, m and v."""
    dt = np.dtype(dtype).type
    out = [np.asarray(a, dt).copy() for a in (p, m, v)]
    new = adam_ref.step(out[0][mask], out[1][mask], out[2][mask], np.asarray(g, dt)[mask], hp, dtype)
    for a, n in zip(out, new):
        a[mask] = n
    return tuple(out)


# ------------------------------------------------------------------ one call of the chain
def chain_step(R, N, F, EM, W, idx, head_step, n_step, gamma, arch, net1, net2, target_net=None, select=True, weight=None,
               adam=None, num_grads=0, period=None, tau=1.0, dtype=np.float64, forced=None):
    """One `optimize_device` call, in the order the chain produces its arrays.

    `R`: the ring's host copy; `idx`: the drawn records; `head_step`: the batched step whose group is being written.
    `net1` / `net2`: dict(sd=state dict (means, `lin_v`, `noisy_sigma`), draw=(seed, stream, counter) of the train copy's
    noise or None[, eps=the vectors themselves]).  `target_net`: None - the toggle, `select` says which network is trained
    (True: net1 on the states, mode 0; False: net2 on the next states, mode 1) -, "max" or "double" (net1 online, net2 the
    target).  `weight`: the importance weights or None.  `adam`: None, or dict(m, v: flat float32 moments of the trained
    network, hp: lr, wd, beta1, beta2, eps of THIS step, step: its number); `num_grads`: gradient steps before this one,
    `period` / `tau`: the target follows when num_grads + 1 is a multiple of `period`.  `forced`: the selections of an
    earlier (fp64) run - dict(trained, other, online: per graph per level, sel) - for the fp32 yardstick run."""
    dt = np.dtype(dtype).type
    R = np.asarray(R, np.float32)
    cap = R.shape[0]
    ns = Nstep(int(n_step), int(W), cap, (int(head_step) % (cap // W)) * W, float(gamma))
    out = dict(mb=nstep_ref.compose(R, N * F, EM, ns, idx))
    mb = out["mb"]
    B = len(idx)
    (sd1, eps1), (sd2, eps2) = (composed(n["sd"], arch, n.get("draw"), n.get("eps")) for n in (net1, net2))
    out.update(sd1=sd1, sd2=sd2, eps1=eps1, eps2=eps2)
    gs, gn = graphs_of(mb, "s", N), graphs_of(mb, "n", N)
    first = target_net is not None or select
    mode = 0 if first else 1
    (sd_t, eps_t, raw_t), sd_o = ((sd1, eps1, net1["sd"]), sd2) if first else ((sd2, eps2, net2["sd"]), sd1)
    g_t, g_o = (gs, gn) if first else (gn, gs)
    fz = forced or {}
    # ---- the forward without gradient, the Double-DQN choice
    r_other = forwards(sd_o, arch, g_o, dtype, fz.get("other"))
    q_t = np.stack([r["out"] for r in r_other])
    out.update(q_t=q_t, runs_other=r_other, mode=mode)
    q_other = q_t
    if target_net == "double":
        r_online = forwards(sd1, arch, gn, dtype, fz.get("online"))
        q_o = np.stack([r["out"] for r in r_online])
        q_sel32, sel, _ = target_net_ref.select(q_o, q_t)
        if "sel" in fz:
            sel = np.asarray(fz["sel"], np.int32)
        value = q_t[np.arange(B), sel]
        q_other = np.repeat(value[:, None], q_t.shape[1], axis=1)
        out.update(q_o=q_o, sel=sel, value=value, q_sel32=q_sel32, runs_online=r_online)
    elif target_net not in (None, "max"):
        raise ValueError("target_net: None, 'max' or 'double'")
    out["q_other"] = q_other
    # ---- the learning step
    r_trained = forwards(sd_t, arch, g_t, dtype, fz.get("trained"))
    ls = learning_step(sd_t, arch["levels"], arch["head"], r_trained, mode, mb["action"], mb["reward"], mb["nonfinal"], gamma,
                       q_other, weight, dtype)
    grads, flat = reduce_grad(ls["steps"], range(B), arch, eps_t, dtype)
    out.update(runs_trained=r_trained, steps=ls["steps"], td=ls["td"], terms=ls["terms"], loss=ls["loss"], grads=grads, flat=flat,
               eps_trained=eps_t)
    # ---- Adam on the trained network, the target's Polyak step
    if adam is not None:
        p0 = flat_of(raw_t, arch, np.float32)
        hp = dict(adam["hp"], step=adam["step"])
        out["p"], out["m"], out["v"] = adam_apply(p0, adam["m"], adam["v"], flat, hp, trained_mask(arch), dtype)
        out["target_after"] = None
        if target_net is not None and period and (int(num_grads) + 1) % int(period) == 0:
            out["target_after"] = target_net_ref.polyak(flat_of(net2["sd"], arch, np.float32), out["p"].astype(np.float32), tau)
    return out


def selections(out):
    """What `forced` takes, from a run."""
    f = dict(trained=[r["perm"] for r in out["runs_trained"]], other=[r["perm"] for r in out["runs_other"]])
    if "sel" in out:
        f.update(online=[r["perm"] for r in out["runs_online"]], sel=out["sel"])
    return f


def _drop_argmax(violations):
    return [m for m in violations if m[0] != "mode1-argmax"]


def margins(o64, o32, arch, factor=KINK):
    """Per graph the decisions of the fp64 run closer than `factor` fp32 yardsticks to flipping: [(what, where, distance,
    yardstick)]; an empty list: the graph's float outputs are continuous in a neighbourhood fp32 arithmetic stays in."""
    B = len(o64["steps"])
    head = types.SimpleNamespace(head=arch["head"])
    out = []
    for b in range(B):
        bad = []
        v = tc.kink_violations(o64["runs_trained"][b], o32["runs_trained"][b], arch["ratio"], factor)
        bad += [("trained",) + m for m in (v if o64["mode"] == 1 else _drop_argmax(v))]
        bad += [("other",) + m for m in _drop_argmax(tc.kink_violations(o64["runs_other"][b], o32["runs_other"][b], arch["ratio"], factor))]
        if "sel" in o64:
            a, c = o64["runs_online"][b], o32["runs_online"][b]
            bad += [("online",) + m for m in _drop_argmax(tc.kink_violations(a, c, arch["ratio"], factor))]
            head.r64, head.r32 = [a], [c]
            gap, yard = dref.argmax_gaps(head)[0]
            if not gap > factor * yard:
                bad.append(("online", "select-argmax", 0, gap, yard))
        dist, yard = abs(abs(float(o64["td"][b])) - 1.0), abs(float(o32["td"][b]) - float(o64["td"][b]))
        if not dist > factor * yard:
            bad.append(("trained", "huber", 0, dist, yard))
        out.append(bad)
    return out


def chain_pair(*args, **kw):
    """(fp64 run, fp32 run forced to its selections, per-graph margins) of `chain_step(*args, **kw)`; both runs carry the
    margins as `margins` and the graphs without a close decision as `keep`."""
    kw.pop("dtype", None), kw.pop("forced", None)
    o64 = chain_step(*args, dtype=np.float64, **kw)
    o32 = chain_step(*args, dtype=np.float32, forced=selections(o64), **kw)
    arch = kw["arch"] if "arch" in kw else args[9]
    mg = margins(o64, o32, arch)
    keep = [b for b, bad in enumerate(mg) if not bad]
    for o in (o64, o32):
        o.update(margins=mg, keep=keep)
    return o64, o32, mg
