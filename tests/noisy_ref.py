"""Restatements of the noisy-network kernels (meshdqn_amd/csrc/mdq_noisy.hip; test helper, numpy and torch on the CPU):
Philox4x32-10, the chain u1, u2 -> z -> eps of include/meshdqn_hip.h in fp64, the float32 composition of a noisy layer and
of its sigma gradient operation by operation, and the fp64 autograd statement of a noisy network through `set_noise`."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
EPS_MAX = 2.41          # |eps| <= sqrt(sqrt(48 ln 2)) = 2.4018...
SEED = 20181            # the noise seed of the GPU tests (test_noisy_net_cpu.py holds its draws to the distribution)
# (stream, draw) pairs of the kernel tests; the first is the one most of them use, the others differ from it in one word each
DRAWS = ((0, 0), (0, 1), (1, 0), (2, (1 << 40) + 5))
# the loop tests: the trainer's default seed 1370 (the default noise seed) and one other noise seed, streams 0 .. 2, one
# draw per step
LOOP_SEEDS, LOOP_STREAMS, LOOP_DRAWS = (1370, 24), (0, 1, 2), 12
# the largest vectors any test asks of (layer, side): lin1 of width 128 reads 256, the families' lin3 has 181 outputs
MAX_LEN = {(0, 0): 256, (0, 1): 128, (1, 0): 128, (1, 1): 64, (2, 0): 64, (2, 1): 181, (3, 0): 64, (3, 1): 1}


def philox4x32_10(counter, key):
    """Philox4x32-10 of Random123: `counter` four and `key` two 32-bit words (numbers or equally shaped integer arrays);
    returns the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK) for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]             # 32 x 32 -> 64 bit: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def noise64(seed, stream, draw, layer, side, n):
    """Entries 0 .. n - 1 of side `side` (0 = in, 1 = out) of noisy layer `layer`: (u1, u2, z, eps) in fp64."""
    j = np.arange(n, dtype=np.uint64)
    r = philox4x32_10((j, 2 * layer + side, draw & MASK, (draw >> 32) & MASK), (seed, stream))
    u1 = ((r[0] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (r[1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return u1, u2, z, np.copysign(np.sqrt(np.abs(z)), z)


def layer_noise64(seed, stream, draw, layout):
    """{layer name: (eps_in, eps_out)} in fp64 for `NodeRemovalNet.noisy_layout()` rows."""
    return {name: (noise64(seed, stream, draw, l, 0, i)[3], noise64(seed, stream, draw, l, 1, o)[3])
            for l, (name, o, i, _, _) in enumerate(layout)}


def compose32(mu_w, mu_b, sig_w, sig_b, eps_in, eps_out):
    """mu + sigma * (eps_out x eps_in) and mu_b + sigma_b * eps_out in float32, every operation rounded on its own, in the
    header's order: (composed weight [out][in], composed bias [out])."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)     # noqa: E731
    mu_w, mu_b, sig_w, sig_b, eps_in, eps_out = map(f, (mu_w, mu_b, sig_w, sig_b, eps_in, eps_out))
    p = (eps_out[:, None] * eps_in[None, :]).astype(np.float32)
    q = (sig_w * p).astype(np.float32)
    return (mu_w + q).astype(np.float32), (mu_b + (sig_b * eps_out).astype(np.float32)).astype(np.float32)


def sigma_grad32(g_w, g_b, eps_in, eps_out):
    """g_w * (eps_out x eps_in) and g_b * eps_out in float32 (what mdq_noisy_grad writes from the means' gradients)."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)     # noqa: E731
    g_w, g_b, eps_in, eps_out = map(f, (g_w, g_b, eps_in, eps_out))
    p = (eps_out[:, None] * eps_in[None, :]).astype(np.float32)
    return (g_w * p).astype(np.float32), (g_b * eps_out).astype(np.float32)


def composed_state_dict(net, noise):
    """State dict of the plain network (no `noisy_sigma`) that the noisy `net` is under `noise` ({layer: (eps_in, eps_out)}
    as float32 arrays): the float32 composition, which the noisy pack is held to bit for bit."""
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if k != "noisy_sigma"}
    sig = net.noisy_sigma.detach().cpu().numpy()
    for name, o, i, off_w, off_b in net.noisy_layout():
        if name not in noise:
            continue
        w, b = compose32(sd[name + ".weight"].numpy(), sd[name + ".bias"].numpy(), sig[off_w:off_w + o * i].reshape(o, i),
                         sig[off_b:off_b + o], *noise[name])
        sd[name + ".weight"], sd[name + ".bias"] = torch.from_numpy(w), torch.from_numpy(b)
    return sd


def autograd64(net, noise, x, src, dst, mask, dout):
    """fp64 autograd through `set_noise` on a double copy of `net`: (outputs, {parameter name: gradient}) of
    sum(forward_dense(...) * dout)."""
    import copy
    n64 = copy.deepcopy(net).double()
    n64.set_noise(noise)
    out = n64.forward_dense(x.double(), src, dst, mask.double())
    (out * torch.as_tensor(dout, dtype=torch.float64)).sum().backward()
    return out.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in n64.named_parameters()}
