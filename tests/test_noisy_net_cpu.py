"""Noisy networks without a GPU: the Python Philox against Random123's known answers, the noise of the GPU tests' draws
against its distribution, the `noisy` option of `NodeRemovalNet` (parameters, bits, `set_noise`, autograd), the ABI of the two
new entry points, and the option's way through `DQNTrainer`, the host loops, train.py and the checkpoint."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import noisy_ref as ref
from test_prioritized_replay_cpu import _c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meshdqn_hip.h")
NAN, INF = float("nan"), float("inf")
OLD_KEYS = ["conv1.lin_l.weight", "conv1.lin_l.bias", "conv1.lin_r.weight", "pool1.weight", "conv2.lin_l.weight",
            "conv2.lin_l.bias", "conv2.lin_r.weight", "pool2.weight", "conv3.lin_l.weight", "conv3.lin_l.bias",
            "conv3.lin_r.weight", "pool3.weight", "conv4.bias", "conv4.lin.weight", "pool4.weight", "conv5.bias",
            "conv5.lin.weight", "pool5.weight", "conv6.bias", "conv6.lin.weight", "pool6.weight", "lin1.weight", "lin1.bias",
            "lin2.weight", "lin2.bias", "lin3.weight", "lin3.bias"]


# ------------------------------------------------------------------ Philox and the noise
def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    f = 0xFFFFFFFF
    assert _hex(ref.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(ref.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(ref.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # arrays in the first counter word give the scalar answers
    r = ref.philox4x32_10((np.array([0, 7, f], np.uint64), 3, 2, 1), (5, 6))
    for k, j in enumerate((0, 7, f)):
        assert [int(w[k]) for w in r] == [int(w) for w in ref.philox4x32_10((j, 3, 2, 1), (5, 6))]


def _held(z, eps, tag):
    n = z.size
    mean, var = float(z.mean()), float(z.var())
    print(f"{tag}: n {n}, mean {mean:+.4f} (bound {5 / math.sqrt(n):.4f}), variance {var:.4f} (1 +- {5 * math.sqrt(2 / n):.4f}), "
          f"largest |eps| {np.abs(eps).max():.4f}")
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1.0) <= 5 * math.sqrt(2 / n), tag
    assert np.abs(eps).max() < ref.EPS_MAX, tag


def test_noise_of_the_gpu_tests_draws_follows_its_distribution():
    """Every value a GPU test can ask for: per noise seed over its (stream, draw) pairs, every (layer, side) at its largest
    length (tests/noisy_ref.py lists them)."""
    sets = {ref.SEED: ref.DRAWS}
    sets.update({s: [(st, d) for st in ref.LOOP_STREAMS for d in range(ref.LOOP_DRAWS)] for s in ref.LOOP_SEEDS})
    for seed, pairs in sets.items():
        zs, es = [], []
        for stream, draw in pairs:
            for (layer, side), n in ref.MAX_LEN.items():
                u1, u2, z, eps = ref.noise64(seed, stream, draw, layer, side, n)
                assert (u1 > 0).all() and (u1 <= 1).all() and (u2 >= 0).all() and (u2 < 1).all()
                zs.append(z), es.append(eps)
        _held(np.concatenate(zs), np.concatenate(es), f"seed {seed}")
    # the bound itself: u1 = 2^-24 and cos = 1
    assert math.sqrt(math.sqrt(48 * math.log(2))) < ref.EPS_MAX
    # another draw, stream, layer or side: other values
    base = ref.noise64(ref.SEED, 0, 0, 0, 0, 64)[3]
    for other in ((ref.SEED, 0, 1, 0, 0), (ref.SEED, 1, 0, 0, 0), (ref.SEED, 0, 0, 1, 0), (ref.SEED, 0, 0, 0, 1),
                  (ref.SEED + 1, 0, 0, 0, 0), (ref.SEED, 0, 1 << 32, 0, 0)):
        assert not np.array_equal(ref.noise64(*other, 64)[3], base), other
    assert np.array_equal(ref.noise64(ref.SEED, 0, 0, 0, 0, 64)[3], base)


# ------------------------------------------------------------------ the module
def _net(head="softmax", noisy=None, out=181, width=128, topk=0.1, seed=11):
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    torch.manual_seed(seed)
    net = NodeRemovalNet(out, conv_width=width, topk=topk, head=head, **({} if noisy is None else dict(noisy=noisy)))
    net.set_num_nodes(17)
    return net


def test_default_network_is_unchanged_and_the_noisy_one_adds_one_parameter_last():
    plain = _net()
    assert sum(p.numel() for p in plain.parameters()) == 173493 and list(plain.state_dict()) == OLD_KEYS
    assert [k for k, _ in plain.named_parameters()] == OLD_KEYS and plain.noisy is None and not hasattr(plain, "noisy_sigma")
    with pytest.raises(ValueError, match="noisy"):
        plain.noisy_layout()
    for head in ("softmax", "linear", "dueling"):
        a, b = _net(head), _net(head, 0.5)
        lay = b.noisy_layout()
        names = ["lin1", "lin2", "lin3"] + (["lin_v"] if head == "dueling" else [])
        assert [r[0] for r in lay] == names
        count, off = 0, 0
        for name, o, i, off_w, off_b in lay:
            assert (o, i) == tuple(getattr(b, name).weight.shape) and off_w == off and off_b == off + o * i
            off += o * i + o
            count += o * i + o
            s = b.noisy_sigma.detach()
            assert torch.equal(s[off_w:off_b + o], torch.full((o * i + o,), 0.5 / math.sqrt(i)))     # constants, per layer
        pa, pb = list(a.named_parameters()), list(b.named_parameters())
        assert [k for k, _ in pb] == [k for k, _ in pa] + ["noisy_sigma"] and pb[-1][1] is b.noisy_sigma
        assert b.noisy_sigma.numel() == count == sum(p.numel() for p in b.parameters()) - sum(p.numel() for p in a.parameters())
        assert [id(p) for p in b.parameters()] == [id(p) for _, p in pb]
        # the flat gradient (the message of the ranks' all-reduce) covers the sigmas, behind the plain network's entries
        assert b.flat_gradients().numel() == a.flat_gradients().numel() + count and not b.flat_gradients()[-count:].any()
        assert set(b.state_dict()) == set(a.state_dict()) | {"noisy_sigma"}
        # the constructor drew the plain network's random numbers: the mean parameters have its bits, and so has the next draw
        assert all(torch.equal(p, q) for (_, p), (_, q) in zip(pa, pb))
        assert len(list(b.parameters())) <= 32
    assert len(list(_net("dueling", 0.5).parameters())) == 30
    torch.manual_seed(5)
    _net("dueling", 0.5, seed=5)
    after_noisy = torch.rand(3)
    torch.manual_seed(5)
    _net("dueling", seed=5)
    assert torch.equal(torch.rand(3), after_noisy)
    for bad in (0, -1.0, NAN, INF, True, "0.5", [0.5]):
        with pytest.raises(ValueError, match="noisy"):
            _net(noisy=bad)
    # a plain checkpoint does not load into a noisy network, nor the other way round
    with pytest.raises(RuntimeError, match="noisy_sigma"):
        _net(noisy=0.5).load_state_dict(_net().state_dict())
    with pytest.raises(RuntimeError, match="noisy_sigma"):
        _net().load_state_dict(_net(noisy=0.5).state_dict())


def _dense_inputs(B=3, n=9, e=20, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, n, 17), generator=g)
    src, dst = torch.randint(0, n, (B, e), generator=g), torch.randint(0, n, (B, e), generator=g)
    mask = (torch.rand((B, e), generator=g) < 0.8).float()
    return x, src, dst, mask


def _noise_for(net, draw=0):
    return ref.layer_noise64(ref.SEED, 0, draw, net.noisy_layout())


@pytest.mark.parametrize("head", ["softmax", "dueling"])
def test_without_noise_the_forward_is_the_plain_networks(head):
    a, b = _net(head, out=21, width=32, topk=0.5), _net(head, 0.5, out=21, width=32, topk=0.5)
    x, src, dst, mask = _dense_inputs()
    with torch.no_grad():
        want = a.forward_dense(x, src, dst, mask)
        assert torch.equal(b.forward_dense(x, src, dst, mask), want)
        b.set_noise(_noise_for(b))
        noisy = b.forward_dense(x, src, dst, mask)
        assert not torch.equal(noisy, want) and torch.isfinite(noisy).all()
        b.set_noise(None)
        assert torch.equal(b.forward_dense(x, src, dst, mask), want)
        # the ragged forward takes the same layers
        from meshdqn_amd.data import Batch, Data
        ei = torch.stack([src[0][mask[0] > 0], dst[0][mask[0] > 0]])
        batch = Batch.from_data_list([Data(x=x[0], edge_index=ei)])
        assert torch.equal(b(batch), a(batch))
        b.set_noise(_noise_for(b))
        assert not torch.equal(b(batch), a(batch))
    with pytest.raises(ValueError, match="set_noise"):
        b.set_noise({"conv1": (np.zeros(17), np.zeros(32))})
    with pytest.raises(ValueError, match="set_noise"):
        b.set_noise({"lin1": (np.zeros(63), np.zeros(128))})
    with pytest.raises(ValueError, match="noisy"):
        a.set_noise({"lin1": (np.zeros(64), np.zeros(128))})


@pytest.mark.parametrize("head", ["softmax", "dueling"])
def test_autograd_of_the_noisy_forward(head):
    """fp64: the outputs are the plain network's with W + S * outer(eps_out, eps_in) in place of W; the gradient of a sigma
    is the gradient of its mean times the noise, which is what mdq_noisy_grad computes from the learning step's gradient."""
    net = _net(head, 0.5, out=21, width=32, topk=0.5)
    with torch.no_grad():       # sigmas that differ from entry to entry
        net.noisy_sigma.mul_(torch.rand(net.noisy_sigma.shape, generator=torch.Generator().manual_seed(9)) + 0.5)
    noise = _noise_for(net, draw=1)
    x, src, dst, mask = _dense_inputs()
    dout = torch.randn((3, 21), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    out, grads = ref.autograd64(net, noise, x, src, dst, mask, dout)
    # ---- the composed plain network
    plain = _net(head, out=21, width=32, topk=0.5).double()
    sd = {k: v.double() for k, v in net.state_dict().items() if k != "noisy_sigma"}
    sig = net.noisy_sigma.detach().double()
    for name, o, i, off_w, off_b in net.noisy_layout():
        e_in, e_out = (torch.from_numpy(e) for e in noise[name])
        sd[name + ".weight"] = sd[name + ".weight"] + sig[off_w:off_w + o * i].view(o, i) * torch.outer(e_out, e_in)
        sd[name + ".bias"] = sd[name + ".bias"] + sig[off_b:off_b + o] * e_out
    plain.load_state_dict(sd)
    want = plain.forward_dense(x.double(), src, dst, mask.double())
    (want * dout).sum().backward()
    assert float((out - want.detach()).abs().max()) <= 1e-12 * max(1.0, float(want.detach().abs().max()))
    gs = grads["noisy_sigma"]
    assert gs is not None and gs.shape == net.noisy_sigma.shape
    for name, o, i, off_w, off_b in net.noisy_layout():
        e_in, e_out = (torch.from_numpy(e) for e in noise[name])
        g_w, g_b = grads[name + ".weight"], grads[name + ".bias"]
        scale = max(1.0, float(g_w.abs().max()))
        assert float(g_w.abs().max()) > 0
        assert float((g_w - getattr(plain, name).weight.grad).abs().max()) <= 1e-12 * scale      # d / d mean = d / d composed
        assert float((gs[off_w:off_w + o * i].view(o, i) - g_w * torch.outer(e_out, e_in)).abs().max()) <= 1e-12 * scale * ref.EPS_MAX ** 2
        assert float((gs[off_b:off_b + o] - g_b * e_out).abs().max()) <= 1e-12 * scale * ref.EPS_MAX
    # the float32 restatements are the fp64 ones rounded operation by operation
    name, o, i, off_w, off_b = net.noisy_layout()[0]
    e_in, e_out = (e.astype(np.float32) for e in noise[name])
    s = net.noisy_sigma.detach().numpy()
    w32, b32 = ref.compose32(net.lin1.weight.detach().numpy(), net.lin1.bias.detach().numpy(), s[off_w:off_w + o * i].reshape(o, i),
                             s[off_b:off_b + o], e_in, e_out)
    assert w32.dtype == b32.dtype == np.float32 and np.abs(w32 - sd["lin1.weight"].numpy()).max() < 1e-5
    assert w32[3, 5] == np.float32(net.lin1.weight[3, 5].item()) + np.float32(np.float32(s[off_w + 3 * i + 5]) * np.float32(e_out[3] * e_in[5]))
    gw32, gb32 = ref.sigma_grad32(grads["lin1.weight"].numpy(), grads["lin1.bias"].numpy(), e_in, e_out)
    assert gw32[3, 5] == np.float32(grads["lin1.weight"][3, 5].item()) * np.float32(e_out[3] * e_in[5]) and gb32.shape == (o,)


# ------------------------------------------------------------------ ABI
CTYPE = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}


def _field_names(header, struct):
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            names += [re.sub(r"\[.*", "", n.strip().split(" ")[-1].lstrip("*")) for n in stmt.split(",")]
    return names


def test_the_entry_points_are_declared_within_abi_8(tmp_path):
    from meshdqn_amd import _lib, build
    header = open(HEADER).read()
    assert _lib.ABI_VERSION == 8 and re.search(r"#define\s+MDQ_ABI_VERSION\s+8\b", header)
    assert sorted(_lib.SYMBOLS) == build.declared_symbols()
    want = {
        "mdq_gcn_pack_noisy": (["const mdq_gcn_pack_table* table", "const mdq_noisy_desc* nz", "void* stream"],
                               [C.c_void_p, C.POINTER(_lib.NoisyDesc), C.c_void_p]),
        "mdq_noisy_grad": (["const mdq_noisy_desc* nz", "const mdq_noisy_grad_layout* lay", "float* grad", "void* stream"],
                           [C.POINTER(_lib.NoisyDesc), C.POINTER(_lib.NoisyGradLayout), C.c_void_p, C.c_void_p]),
    }
    for name, (args, ctypes_) in want.items():
        assert name in _lib.SYMBOLS and name in build.declared_symbols()
        decl = re.search(r"MDQ_API int " + name + r"\(([^)]*)\)", header).group(1)
        assert [" ".join(a.split()) for a in decl.split(",")] == args
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and list(argtypes) == ctypes_
    assert int(re.search(r"#define\s+MDQ_NOISY_MAX\s+(\d+)", header).group(1)) == _lib.NOISY_MAX == 4
    # the descriptors: field names and order from the header's text, sizes and offsets from the compiler
    f = _lib.NoisyDesc._fields_
    assert _field_names(header, "mdq_noisy_desc") == [n for n, _ in f] == \
        ["n", "_pad", "seed", "stream", "draw", "seg_w", "seg_b", "sigma_w", "sigma_b", "eps_in", "eps_out"]
    assert [t for _, t in f] == [C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int32 * 4, C.c_int32 * 4] + \
        [C.c_void_p * 4] * 4
    size, c_off, py_off = _c_layout(tmp_path, "mdq_noisy_desc", _lib.NoisyDesc)
    assert size == C.sizeof(_lib.NoisyDesc) == 8 + 8 + 8 + 32 + 4 * 32 and c_off == py_off
    f = _lib.NoisyGradLayout._fields_
    assert _field_names(header, "mdq_noisy_grad_layout") == [n for n, _ in f] == \
        ["total", "_pad", "out", "in", "mu_w", "mu_b", "sig_w", "sig_b"]
    assert [t for _, t in f] == [C.c_int32, C.c_int32] + [C.c_int32 * 4] * 6
    size, c_off, py_off = _c_layout(tmp_path, "mdq_noisy_grad_layout", _lib.NoisyGradLayout)
    assert size == C.sizeof(_lib.NoisyGradLayout) == 8 + 6 * 16 and c_off == py_off
    # the pack's own table and entry point are what they were
    from meshdqn_amd.gcn_fused import GcnPackTable
    size, c_off, py_off = _c_layout(tmp_path, "mdq_gcn_pack_table", GcnPackTable)
    assert size == C.sizeof(GcnPackTable) == 8 + 256 + 256 + 128 + 128 and c_off == py_off
    assert re.search(r"MDQ_API int mdq_gcn_pack\(const mdq_gcn_pack_table\* table, void\* stream\);", header)
    # a unit of its own, which includes no other .hip file
    assert build.UNITS["noisy"] == ("mdq_noisy.hip", [], [])
    # the header names the float functions and the bound
    text = re.search(r"Noisy-network exploration.*?#define MDQ_NOISY_MAX", header, flags=re.S).group(0)
    for word in ("Philox4x32-10", "logf", "sqrtf", "cospif", "copysignf", "2.41", "no fused multiply-add"):
        assert word in text, word


# ------------------------------------------------------------------ the option
def _trainer(**kw):
    from meshdqn_amd.trainer import DistContext, DQNTrainer
    return DQNTrainer(n_actions=20, num_inputs=17, ctx=DistContext(device=torch.device("cpu")), conv_width=32, **kw)


def test_trainer_validates_the_option():
    base = _trainer()
    assert base.noisy is None and _trainer(noisy=None).noisy is None
    assert base.policy_net_1.noisy is None and not hasattr(base.policy_net_1, "noisy_sigma")
    assert _trainer(noisy={}).noisy == dict(sigma0=0.5, seed=1370)                  # the trainer's default seed
    assert _trainer(noisy={}, seed=7).noisy == dict(sigma0=0.5, seed=7)
    assert _trainer(noisy=dict(sigma0=1, seed=np.int64(9))).noisy == dict(sigma0=1.0, seed=9)
    for bad in (dict(sigma0=0), dict(sigma0=-0.5), dict(sigma0=NAN), dict(sigma0=INF), dict(sigma0=True), dict(sigma0="0.5"),
                dict(sigma0=None), dict(seed=-1), dict(seed=2 ** 32), dict(seed=1.5), dict(seed=True), dict(seed="3"),
                dict(sigma=0.5), dict(sigma0=0.5, period=3), 0.5, True, "on", [0.5]):
        with pytest.raises(ValueError, match="noisy"):
            _trainer(noisy=bad)
    tr = _trainer(noisy=dict(sigma0=0.25), head="dueling", target_net=dict(kind="double"))
    for net in (tr.policy_net_1, tr.policy_net_2):
        assert net.noisy == 0.25 and [r[0] for r in net.noisy_layout()] == ["lin1", "lin2", "lin3", "lin_v"]
        assert float(net.noisy_sigma.detach()[0]) == np.float32(0.25 / math.sqrt(64)) and len(list(net.parameters())) == 30
    assert torch.equal(tr.policy_net_1.noisy_sigma, tr.policy_net_2.noisy_sigma)
    # both networks have the bits of the plain trainer's from the same seed, and both optimisers hold the sigmas
    plain, noisy = _trainer(), _trainer(noisy={})
    for a, b in ((plain.policy_net_1, noisy.policy_net_1), (plain.policy_net_2, noisy.policy_net_2)):
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert all(any(p is n.noisy_sigma for p in o.param_groups[0]["params"])
               for o, n in zip(noisy.opts, (noisy.policy_net_1, noisy.policy_net_2)))
    assert noisy.noise_draws == dict(act1=0, train1=0, train2=0) and noisy.NOISE_COPIES == ("act1", "train1", "train2")


def test_the_host_paths_refuse_the_trainer():
    from meshdqn_amd.trainer import train_loop_per_worker, train_loop_vec
    tr = _trainer(noisy={})
    with pytest.raises(ValueError, match="train_loop_device"):
        train_loop_vec(tr, None, 3)
    with pytest.raises(ValueError, match="train_loop_device"):
        train_loop_per_worker(tr, None, 1)
    with pytest.raises(ValueError, match="train_loop_device"):
        tr.optimize()
    from meshdqn_amd.gcn_fused import FusedGcn
    fg = FusedGcn.__new__(FusedGcn)             # (no library needed for the refusal)
    fg.net = _trainer().policy_net_1
    with pytest.raises(ValueError, match="noisy"):
        fg.resample(1, 0, 0)


def test_train_script_parses_the_flag_and_the_yaml_block():
    import yaml
    spec = importlib.util.spec_from_file_location("mdq_train_script", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    cfg_path = os.path.join(ROOT, "configs", "ray_ys930.yaml")
    cfg = yaml.safe_load(open(cfg_path))

    def flag(*extra):
        return train.parser().parse_args(["--config", cfg_path, *extra]).noisy_net
    assert flag() is None and "noisy_net" not in cfg and train.noisy_options(flag(), cfg) is None
    assert train.noisy_options(flag("--noisy-net"), cfg) == {}
    assert train.noisy_options(flag("--noisy-net", "0.25"), cfg) == dict(sigma0=0.25)
    assert train.noisy_options(flag("--noisy-net", "1"), cfg) == dict(sigma0=1.0)
    assert train.parser().parse_args(["--config", cfg_path, "--noisy-net", "--envs", "4"]).envs == 4
    with pytest.raises(SystemExit):
        flag("--noisy-net", "loud")
    block = yaml.safe_load("noisy_net: {sigma0: 0.1}")
    assert train.noisy_options(flag(), block) == dict(sigma0=0.1)
    assert train.noisy_options(flag("--noisy-net"), block) == dict(sigma0=0.1)
    assert train.noisy_options(flag("--noisy-net", "0.3"), block) == dict(sigma0=0.3)
    assert train.noisy_options(flag(), yaml.safe_load("noisy_net: {}")) == {}
    assert _trainer(noisy=train.noisy_options(flag("--noisy-net"), cfg), seed=3).noisy == dict(sigma0=0.5, seed=3)
    assert _trainer(noisy=train.noisy_options(flag(), block)).noisy == dict(sigma0=0.1, seed=1370)
    with pytest.raises(SystemExit, match="noisy_net"):
        train.noisy_options(flag(), yaml.safe_load("noisy_net: {sigma0: 0.5, seed: 3}"))
    with pytest.raises(SystemExit, match="noisy_net"):
        train.noisy_options(flag(), yaml.safe_load("noisy_net: 0.5"))
    with pytest.raises(ValueError, match="sigma0"):
        _trainer(noisy=train.noisy_options(flag("--noisy-net", "0"), cfg))


def test_checkpoint_keeps_the_draw_counters(tmp_path):
    a = _trainer(noisy=dict(sigma0=0.25))
    with torch.no_grad():
        a.policy_net_1.noisy_sigma.mul_(1.5)
    a.noise_draws.update(act1=40, train1=(1 << 40) + 3, train2=38)
    a.num_grads = 13
    a.save(str(tmp_path), "n_")
    st = torch.load(os.path.join(str(tmp_path), "n_trainer_state.pt"), weights_only=True)
    assert st["noise_draws"] == dict(act1=40, train1=(1 << 40) + 3, train2=38)
    b = _trainer(noisy=dict(sigma0=0.25))
    b.load(str(tmp_path), "n_")
    assert b.noise_draws == a.noise_draws and b.num_grads == 13
    assert torch.equal(b.policy_net_1.noisy_sigma, a.policy_net_1.noisy_sigma)
    assert not torch.equal(b.policy_net_1.noisy_sigma, b.policy_net_2.noisy_sigma)
    # a plain trainer writes no counters, and its checkpoint does not load into a noisy one (nor the noisy one into it)
    plain = _trainer()
    plain.save(str(tmp_path), "p_")
    assert "noise_draws" not in torch.load(os.path.join(str(tmp_path), "p_trainer_state.pt"), weights_only=True)
    with pytest.raises(RuntimeError, match="noisy_sigma"):
        _trainer(noisy={}).load(str(tmp_path), "p_")
    with pytest.raises(RuntimeError, match="noisy_sigma"):
        _trainer().load(str(tmp_path), "n_")
