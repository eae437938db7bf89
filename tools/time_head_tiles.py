"""A / B of the Q-head kernels (dev tool): `forward_arrays` of 128 graphs (180 nodes, ~400 edges each, the env step's shapes)
with MDQ_HEAD_TILES=32 (mlp_head_c128_kernel, 32-graph tiles) against the default (mlp_head_c128_t16_kernel), alternately in
one process; HIP events around every call, 200 calls per setting after a warm-up.  The embedding kernel is part of both.
--q-head {softmax,linear,dueling}: the head of the network (default softmax).
--noisy-net: a noisy network (sigma0 0.5) whose copy is resampled in front of every forward (mdq_gcn_pack_noisy is then part
of every timed call); the outputs are compared on one fixed draw."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from meshdqn_amd.airfoilgcnn import NodeRemovalNet
from meshdqn_amd.gcn_fused import FusedGcn
B, N, E, F, CALLS = 128, 180, 400, 17, 200
rng = np.random.default_rng(5)
HEAD = sys.argv[sys.argv.index("--q-head") + 1] if "--q-head" in sys.argv else "softmax"
NOISY = "--noisy-net" in sys.argv
net = NodeRemovalNet(181, conv_width=128, topk=0.1, head=HEAD, noisy=0.5 if NOISY else None); net.set_num_nodes(F); fused = FusedGcn(net.cuda())
draws = iter(range(1, 1 << 30))
x = torch.from_numpy(rng.standard_normal((B * N, F))).float().cuda()
node_ptr = torch.arange(B + 1, dtype=torch.int32, device="cuda") * N
edge_ptr = torch.arange(B + 1, dtype=torch.int32, device="cuda") * E
esrc = torch.from_numpy(rng.integers(0, N, B * E)).to(torch.int32).cuda()
edst = torch.from_numpy(rng.integers(0, N, B * E)).to(torch.int32).cuda()
def call(draw=None):
    if NOISY:
        fused.resample(5, 0, next(draws) if draw is None else draw)
    return fused.forward_arrays(x, node_ptr, esrc, edst, edge_ptr, N, E)
def timed(n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
res, outs = {"32": [], "16": []}, {}
for rnd in range(5):            # alternate the settings: 5 x 40 calls each
    for tiles in ("32", "16"):
        if tiles == "32":
            os.environ["MDQ_HEAD_TILES"] = "32"
        else:
            os.environ.pop("MDQ_HEAD_TILES", None)
        timed(20)
        res[tiles].append(timed(CALLS // 5))
        outs[tiles] = call(0).cpu().numpy()
print("outputs bitwise equal:", bool(np.array_equal(outs["32"].view(np.uint32), outs["16"].view(np.uint32))))
for tiles in ("32", "16"):
    t = np.concatenate(res[tiles])
    print(f"q_head {HEAD}, noisy {NOISY}, head tiles {tiles}: forward_arrays of {B} graphs, {t.size} calls: mean {t.mean():.2f} us, median {np.median(t):.2f} us, min {t.min():.2f} us")
