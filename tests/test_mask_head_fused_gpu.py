"""The mask head's up-sampling depthwise conv and its 256 -> 32 projection as one kernel (ops.dwconv5x5_up2_pw ->
mdqe_dwconv5x5_up2_pw_c256_f32) against the two launches it replaces (ops.dwconv5x5(up2=True), then ops.linear): torch.equal.

Equal bits are by construction -- the depthwise values are the same expressions, and the product accumulates over k in the order of the
K-step-16 GEMM kernel from a zero accumulator with bias added last -- so nothing here has a tolerance.  Shapes (NI, Hs, Ws), the
smallest at which the kernel can go wrong: one quad; all-border rows and columns; a quad count that is no multiple of a wave's strip of
8 quads ((2,3,3): 18 quads in 6 strips of 3; (1,2,9): strips of 8 + 1); (3,12,20): interior quads, strips of 8 + 8 + 4, more strips (108)
than one block's four waves.  The result goes into a row range of a larger buffer and into a buffer with a wider row pitch; what lies
outside must keep a canary.  Everything the fused kernel does not take (other widths, the split-precision GEMM modes, the switch off)
must give the two launches' bits because it IS the two launches.

Wall time on one MI355X: a fraction of a second per case; the engine case builds one R50 engine with one encoder / decoder layer.
"""
import dataclasses
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 3, 3), (1, 2, 9), (3, 12, 20)]
CANARY = -12345.0


def _weights(C, N, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(wt=(r(25, C) * 0.2).cuda(), bias=r(C).cuda(), tw=(1.0 + 0.3 * r(C)).cuda(), tb=r(C).cuda(),
                pw=(r(N, C) / C ** 0.5).cuda(), pb=r(N).cuda())


def _input(NI, Hs, Ws, C, seed):
    return torch.randn(NI, Hs, Ws, C, generator=torch.Generator().manual_seed(seed)).cuda()


def _two_launches(ops, x, p, out=None):
    z = ops.dwconv5x5(x, p["wt"], p["bias"], up2=True, tw=p["tw"], tb=p["tb"])
    return ops.linear(z.view(-1, z.shape[-1]), p["pw"], p["pb"], out=out)


def _fused(ops, x, p, out=None):
    return ops.dwconv5x5_up2_pw(x, p["wt"], p["bias"], p["tw"], p["tb"], p["pw"], p["pb"], out=out)


def _count_fused_calls(monkeypatch):
    """-> a one-element list that counts the calls of the fused entry point from here on."""
    from mdqe_cvpr2023_amd import ops
    calls = [0]
    real = ops.lib.mdqe_dwconv5x5_up2_pw_c256_f32

    class Lib:
        def __getattr__(self, name):
            return getattr(ops_lib, name)

        def mdqe_dwconv5x5_up2_pw_c256_f32(self, *a):
            calls[0] += 1
            return real(*a)

    ops_lib = ops.lib
    monkeypatch.setattr(ops, "lib", Lib())
    return calls


@pytest.mark.parametrize("NI,Hs,Ws", SHAPES)
def test_fused_kernel_has_the_two_launches_bits(monkeypatch, NI, Hs, Ws):
    from mdqe_cvpr2023_amd import ops
    p = _weights(256, 32, seed=Hs * 100 + Ws)
    x = _input(NI, Hs, Ws, 256, seed=NI)
    want = _two_launches(ops, x, p)
    calls = _count_fused_calls(monkeypatch)
    got = _fused(ops, x, p)
    again = _fused(ops, x, p)
    torch.cuda.synchronize()
    assert calls[0] == 2                                             # the one kernel ran, not the two launches
    assert got.shape == want.shape == (NI * 4 * Hs * Ws, 32)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0.1
    assert torch.equal(got, want)
    assert torch.equal(again, got)


@pytest.mark.parametrize("NI,Hs,Ws", [(2, 3, 3), (3, 12, 20)])
def test_fused_kernel_stores_into_a_view_and_nowhere_else(monkeypatch, NI, Hs, Ws):
    from mdqe_cvpr2023_amd import ops
    p = _weights(256, 32, seed=7)
    x = _input(NI, Hs, Ws, 256, seed=8)
    rows = NI * 4 * Hs * Ws
    want = _two_launches(ops, x, p)
    calls = _count_fused_calls(monkeypatch)
    # a row range of a larger buffer (what the frame cache passes)
    big = torch.full((rows + 24, 32), CANARY, device="cuda")
    assert _fused(ops, x, p, out=big[16:16 + rows]).data_ptr() == big[16:].data_ptr()
    assert torch.equal(big[16:16 + rows], want)
    assert bool((big[:16] == CANARY).all()) and bool((big[16 + rows:] == CANARY).all())
    # rows 40 floats apart: the columns past 32 are not the kernel's
    wide = torch.full((rows, 40), CANARY, device="cuda")
    _fused(ops, x, p, out=wide[:, :32])
    assert torch.equal(wide[:, :32], want) and bool((wide[:, 32:] == CANARY).all())
    assert calls[0] == 2


def test_everything_else_keeps_the_two_launches(monkeypatch):
    from mdqe_cvpr2023_amd import ops
    calls = _count_fused_calls(monkeypatch)
    x = _input(2, 3, 5, 256, seed=1)
    for C, N in ((256, 24), (192, 32)):                              # another projection width; another channel count (Swin-L's head)
        p = _weights(C, N, seed=C + N)
        xc = x[..., :C].contiguous()
        assert torch.equal(_fused(ops, xc, p), _two_launches(ops, xc, p))
    p = _weights(256, 32, seed=3)
    with ops.gemm_precision("f16x3"):                                # the split-precision product is not the fused kernel's sum
        assert torch.equal(_fused(ops, x, p), _two_launches(ops, x, p))
    off = torch.empty(x.numel() // 256 * 4 * 32 + 1, device="cuda")[1:].view(-1, 32)   # `out` 4 bytes off a 16-byte boundary
    assert torch.equal(_fused(ops, x, p, out=off), _two_launches(ops, x, p))
    monkeypatch.setattr(ops, "MASK_HEAD_FUSED", False)               # what MDQE_MASK_HEAD_FUSED=0 sets
    assert torch.equal(_fused(ops, x, p), _two_launches(ops, x, p))
    assert calls[0] == 0
    monkeypatch.setattr(ops, "MASK_HEAD_FUSED", True)
    assert torch.equal(_fused(ops, x, p), _two_launches(ops, x, p))
    assert calls[0] == 1


def test_engine_mask_features_equal_with_the_switch_on_and_off(monkeypatch):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.engine import Engine
    from mdqe_cvpr2023_amd.params import random_state
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], enc_layers=1, dec_layers=1)
    sd = random_state(cfg, seed=4)
    g = torch.Generator().manual_seed(9)
    for k in sd:                                                     # (random_state leaves the head's biases at zero)
        if ("out_lay2" in k or "out_uplay" in k) and sd[k].dim() == 1:
            sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g)
    eng = Engine(cfg, sd)
    geo = eng.geometry(64, 96)
    enc = torch.randn(2, geo.N, cfg.hidden_dim, generator=g).cuda()
    Hm, Wm, Md = eng.mask_feature_shape(geo)
    assert Md == 32
    calls = _count_fused_calls(monkeypatch)
    outs = []
    with torch.no_grad():
        for flag in (True, False):
            monkeypatch.setattr(ops, "MASK_HEAD_FUSED", flag)
            ring = torch.full((5, Hm, Wm, Md), CANARY, device="cuda")
            mf = eng.mask_features(enc, geo, out=ring[1:3])
            assert mf.data_ptr() == ring[1:].data_ptr()
            assert bool((ring[0] == CANARY).all()) and bool((ring[3:] == CANARY).all())
            outs.append((ring[1:3].clone(), eng.mask_features(enc, geo)))
    assert calls[0] == 2                                             # with and without `out`, switch on
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][0], outs[0][1])
