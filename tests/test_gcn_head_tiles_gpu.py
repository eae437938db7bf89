"""GPU: the Q-head on 16-graph tiles (`mlp_head_c128_t16_kernel`, the default for conv width 128) against the 32-graph tiles
of `mlp_head_c128_kernel` (MDQ_HEAD_TILES=32) on the same inputs.  Both kernels run the same sequential fma chain over k per
output (v_mfma_f32_16x16x4_f32 / 32x32x2_f32, tools/micro/mfma_exact.hip), so the outputs must be BITWISE equal - at every
tile edge of either kernel: 1, 15, 16, 17 and 33 graphs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OUT_DIM, FEAT = 181, 17


@pytest.fixture(scope="module")
def fused(lib_built):
    """NodeRemovalNet at the reference's width with seeded random weights, and its packed device copy."""
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    from meshdqn_amd.gcn_fused import FusedGcn
    rng = np.random.default_rng(1605)
    net = NodeRemovalNet(output_dim=OUT_DIM, conv_width=128, topk=0.1)
    net.set_num_nodes(FEAT)
    sd = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape)) * 0.3).float() for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    return FusedGcn(net.cuda())


def _batch(B):
    from meshdqn_amd.data import Batch, Data
    rng = np.random.default_rng(100 + B)
    graphs = []
    for g in range(B):
        n, e = int(rng.integers(20, 48)), int(rng.integers(30, 90))
        graphs.append(Data(x=torch.from_numpy(rng.standard_normal((n, FEAT))).float(),
                           edge_index=torch.from_numpy(rng.integers(0, n, size=(2, e))).long()))
    return Batch.from_data_list(graphs).to("cuda")


@pytest.mark.parametrize("B,softmax", [(1, 0), (15, 0), (16, 0), (17, 0), (33, 0), (33, 1)])
def test_head_on_16_graph_tiles_is_bitwise_the_32_graph_head(fused, monkeypatch, B, softmax):
    batch = _batch(B)
    fused._pack()
    fused.desc.softmax = softmax        # (the head's last stage; the packed table is rebuilt only when the parameters move)
    assert fused.desc.C == 128 and fused.desc.out_dim == OUT_DIM
    monkeypatch.setenv("MDQ_HEAD_TILES", "32")
    q32, e32 = fused.forward(batch, return_embedding=True)
    monkeypatch.delenv("MDQ_HEAD_TILES")
    q16, e16 = fused.forward(batch, return_embedding=True)
    torch.cuda.synchronize()
    q32, q16, e32, e16 = (t.cpu().numpy() for t in (q32, q16, e32, e16))
    assert q16.shape == (B, OUT_DIM) and np.isfinite(q32).all() and np.isfinite(q16).all()
    assert np.array_equal(e32.view(np.uint32), e16.view(np.uint32))       # the same inputs of the head
    assert np.ptp(q32, axis=1).min() > 0                                  # (rows that say something)
    if softmax:
        assert np.abs(q32.sum(1) - 1).max() < 1e-5
    bad = q32.view(np.uint32) != q16.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(q32 - q16).max()))
