"""GPU numerics of the dense HIP kernels vs a plain PyTorch fp32 (CPU) reference of the same op.
Tolerance: exact-fp32 MFMA accumulates in a different order than the CPU BLAS; 2e-5 relative to the
output scale (the path's bar is 1e-3)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@pytest.mark.parametrize("M,N,K,tile", [(1000, 384, 256, 0), (5100 * 2, 640, 256, 1), (777, 256, 1024, 1), (784, 256, 256, 3),
                                        (196, 25, 256, 0), (130, 4, 256, 3), (4100, 64, 64, 2), (300, 96, 36, 0), (64, 1, 256, 0),
                                        (257, 129, 100, 0)])
def test_gemm(M, N, K, tile):
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    ref = F.linear(x, w, b)
    out = ops.linear(x.cuda(), w.cuda(), b.cuda(), tile=tile).cpu()
    assert rel(out, ref) < 2e-5


def test_gemm_epilogues():
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(5)
    M, N, K = 700, 640, 256
    x = torch.randn(M, K, generator=g); w = torch.randn(N, K, generator=g) / 16; b = torch.randn(N, generator=g)
    res = torch.randn(100, N, generator=g)
    mask = torch.rand(M, generator=g) < 0.2
    ref = F.linear(x, w, b)
    ref[:, :300] = F.gelu(ref[:, :300])
    ref = ref + res[torch.arange(M) % 100]
    ref[:, :256] = ref[:, :256].masked_fill(mask[:, None], 0.0)
    out = ops.linear(x.cuda(), w.cuda(), b.cuda(), act="gelu", act_cols=300, residual=res.cuda(), res_mod=100,
                     rowmask=mask.cuda(), mask_cols=256).cpu()
    assert rel(out, ref) < 2e-5
    # strided input rows + strided output (writing into a wider buffer)
    big = torch.randn(M, 2 * K, generator=g)
    outbuf = torch.zeros(M, 1000).cuda()
    ops.linear(big.cuda()[:, K:], w.cuda(), None, act="relu", out=outbuf[:, 100:100 + N], ldc=1000)
    ref2 = F.relu(F.linear(big[:, K:], w))
    assert rel(outbuf[:, 100:100 + N].cpu(), ref2) < 2e-5
    assert float(outbuf[:, :100].abs().max()) == 0.0 and float(outbuf[:, 100 + N:].abs().max()) == 0.0


@pytest.mark.parametrize("NI,H,W,Cin,Cout,k,s,p", [(2, 24, 40, 64, 64, 3, 1, 1), (2, 24, 40, 128, 96, 3, 2, 1), (3, 12, 20, 256, 256, 3, 1, 1),
                                                   (1, 13, 21, 64, 256, 1, 1, 0), (2, 12, 20, 512, 128, 1, 2, 0), (1, 6, 10, 2048, 256, 3, 2, 1),
                                                   (1, 9, 7, 32, 40, 5, 1, 2)])
def test_conv(NI, H, W, Cin, Cout, k, s, p):
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(H * W + Cin)
    x = torch.randn(NI, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g)
    ref = F.relu(F.conv2d(x, w, b, s, p))
    res = torch.randn_like(ref)
    ref2 = F.relu(F.conv2d(x, w, b, s, p) + res) if False else None
    xg = x.permute(0, 2, 3, 1).contiguous().cuda()
    wg = w.permute(0, 2, 3, 1).contiguous().cuda()
    out = ops.conv2d_nhwc(xg, wg, b.cuda(), s, p, act="relu").cpu().permute(0, 3, 1, 2)
    assert out.shape == ref.shape
    assert rel(out, ref) < 2e-5
    # residual added AFTER the activation slot is the kernel's order; bottleneck uses act=None + residual then relu elsewhere
    out3 = ops.conv2d_nhwc(xg, wg, b.cuda(), s, p, act=None, residual=res.permute(0, 2, 3, 1).contiguous().cuda()).cpu().permute(0, 3, 1, 2)
    assert rel(out3, F.conv2d(x, w, b, s, p) + res) < 2e-5


@pytest.mark.parametrize("C", [256, 192, 64, 1024])
def test_layernorm(C):
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(C)
    x = torch.randn(1001, C, generator=g) * 3 + 1
    r = torch.randn(1001, C, generator=g)
    ga, be = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x + r, (C,), ga, be, 1e-5)
    out = ops.layernorm(x.cuda(), ga.cuda(), be.cuda(), res=r.cuda()).cpu()
    assert float((out - ref).abs().max()) < 2e-5
    out = ops.layernorm(x.cuda(), ga.cuda(), be.cuda()).cpu()
    assert float((out - F.layer_norm(x, (C,), ga, be, 1e-5)).abs().max()) < 2e-5


@pytest.mark.parametrize("NI,HW,C,G,act", [(3, 3840, 256, 32, None), (2, 240, 256, 8, "gelu"), (2, 15360, 32, 32, "relu"), (2, 60, 192, 24, None),
                                           (1, 7, 24, 24, "relu")])
def test_groupnorm(NI, HW, C, G, act):
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(HW + C)
    x = torch.randn(NI, HW, C, generator=g) * 2 + 0.7
    ga, be = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.group_norm(x.permute(0, 2, 1), G, ga, be, 1e-5)
    if act == "gelu":
        ref = F.gelu(ref)
    elif act == "relu":
        ref = F.relu(ref)
    out = ops.groupnorm_nhwc(x.cuda(), G, ga.cuda(), be.cuda(), act=act).cpu().permute(0, 2, 1)
    assert float((out - ref).abs().max()) < 3e-5


def test_stem_maxpool_upsample_dw():
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(9)
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    for dt in (torch.uint8, torch.float32):
        fr = torch.randint(0, 256, (2, 3, 60, 90), generator=g).to(dt)
        xn = (fr.float() - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
        xp = torch.zeros(2, 3, 64, 96); xp[:, :, :60, :90] = xn
        w = torch.randn(64, 3, 7, 7, generator=g) / 12
        ref = F.conv2d(xp, w, None, 2, 3)
        col = ops.stem_im2col(fr.cuda(), 64, 96, mean, std)
        wp = torch.zeros(64, 160); wp[:, :147] = w.permute(0, 2, 3, 1).reshape(64, 147)
        out = ops.linear(col, wp.cuda()).view(2, 32, 48, 64).cpu().permute(0, 3, 1, 2)
        assert rel(out, ref) < 2e-5
        # the fused stem (no im2col buffer): same conv + bias + ReLU in one kernel
        b = torch.randn(64, generator=g)
        wk = ops.stem_weight_kmajor(w.permute(0, 2, 3, 1).contiguous())
        out = ops.stem_conv(fr.cuda(), 64, 96, mean, std, wk.cuda(), b.cuda()).cpu().permute(0, 3, 1, 2)
        assert rel(out, F.relu(ref + b.view(1, 64, 1, 1))) < 2e-5
    # fused stem: ragged tiles (output 36 x 44 is not a multiple of the 8 x 16 tile).  45 tiles on 45 blocks: every block walks ONE tile;
    # the persistent loop and its register prefetch run in tests/test_conv_spatial_gpu.py (1560 tiles on 768 blocks)
    fr = torch.randint(0, 256, (3, 3, 70, 85), generator=g).to(torch.uint8)
    xn = (fr.float() - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    xp = torch.zeros(3, 3, 72, 88); xp[:, :, :70, :85] = xn
    w = torch.randn(64, 3, 7, 7, generator=g) / 12; b = torch.randn(64, generator=g)
    ref = F.relu(F.conv2d(xp, w, b, 2, 3))
    out = ops.stem_conv(fr.cuda(), 72, 88, mean, std, ops.stem_weight_kmajor(w.permute(0, 2, 3, 1).contiguous()).cuda(), b.cuda())
    assert rel(out.cpu().permute(0, 3, 1, 2), ref) < 2e-5
    x = torch.randn(2, 64, 31, 48, generator=g)
    out = ops.maxpool3x3s2(x.permute(0, 2, 3, 1).contiguous().cuda()).cpu().permute(0, 3, 1, 2)
    assert torch.equal(out, F.max_pool2d(x, 3, 2, 1))
    a = torch.randn(2, 32, 24, 40, generator=g); b = torch.randn(2, 32, 12, 20, generator=g)
    out = ops.upsample_nearest_add(a.permute(0, 2, 3, 1).contiguous().cuda(), b.permute(0, 2, 3, 1).contiguous().cuda()).cpu().permute(0, 3, 1, 2)
    assert torch.equal(out, a + F.interpolate(b, size=(24, 40), mode="nearest"))
    b2 = torch.randn(2, 32, 7, 9, generator=g); a2 = torch.randn(2, 32, 15, 20, generator=g)
    out = ops.upsample_nearest_add(a2.permute(0, 2, 3, 1).contiguous().cuda(), b2.permute(0, 2, 3, 1).contiguous().cuda()).cpu().permute(0, 3, 1, 2)
    assert torch.equal(out, a2 + F.interpolate(b2, size=(15, 20), mode="nearest"))
    # depthwise 5x5 and the fused (transposed-conv x2 -> depthwise 5x5)
    C = 32
    x = torch.randn(2, C, 12, 20, generator=g)
    dw = torch.randn(C, 1, 5, 5, generator=g) / 5; db = torch.randn(C, generator=g)
    ref = F.conv2d(x, dw, db, padding=2, groups=C)
    xg = x.permute(0, 2, 3, 1).contiguous().cuda()
    wt = dw.view(C, 25).t().contiguous().cuda()
    out = ops.dwconv5x5(xg, wt, db.cuda()).cpu().permute(0, 3, 1, 2)
    assert rel(out, ref) < 1e-5
    tw = torch.randn(C, 1, 1, 1, generator=g); tb = torch.randn(C, generator=g)
    up = F.conv_transpose2d(x, tw, tb, stride=2, output_padding=1, groups=C)
    ref = F.conv2d(up, dw, db, padding=2, groups=C)
    out = ops.dwconv5x5(xg, wt, db.cuda(), up2=True, tw=tw.view(C).cuda(), tb=tb.cuda()).cpu().permute(0, 3, 1, 2)
    assert out.shape == ref.shape and rel(out, ref) < 1e-5
    # C == 256: the register-tap depthwise kernel (odd width: the pair loop's tail) and the quad form of
    # ConvTranspose x2 -> depthwise 5x5 (tiny images: every quad is a border quad; and a larger one)
    C = 256
    for (H, W) in ((2, 3), (7, 9), (12, 20)):
        x = torch.randn(2, C, H, W, generator=g)
        dw = torch.randn(C, 1, 5, 5, generator=g) / 5; db = torch.randn(C, generator=g)
        xg = x.permute(0, 2, 3, 1).contiguous().cuda()
        wt = dw.view(C, 25).t().contiguous().cuda()
        out = ops.dwconv5x5(xg, wt, db.cuda()).cpu().permute(0, 3, 1, 2)
        assert rel(out, F.conv2d(x, dw, db, padding=2, groups=C)) < 1e-5
        tw = torch.randn(C, 1, 1, 1, generator=g); tb = torch.randn(C, generator=g)
        up = F.conv_transpose2d(x, tw, tb, stride=2, output_padding=1, groups=C)
        ref = F.conv2d(up, dw, db, padding=2, groups=C)
        out = ops.dwconv5x5(xg, wt, db.cuda(), up2=True, tw=tw.view(C).cuda(), tb=tb.cuda())
        assert tuple(out.shape) == (2, 2 * H, 2 * W, C)
        assert rel(out.cpu().permute(0, 3, 1, 2), ref) < 1e-5
        ops.DW_FAST = False                                  # the generic kernel (other channel counts take it) agrees
        try:
            two = ops.dwconv5x5(xg, wt, db.cuda(), up2=True, tw=tw.view(C).cuda(), tb=tb.cuda())
        finally:
            ops.DW_FAST = True
        assert rel(out, two) < 1e-5


def test_gemm_splitk_and_mask_stats():
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(3)
    a = torch.rand(150, 15360, generator=g); b = (torch.rand(150, 15360, generator=g) > 0.5).float()
    ref = a @ b.t()
    out = ops.linear(a.cuda(), b.cuda()).cpu()                    # auto split-K
    assert rel(out, ref) < 2e-5
    out = ops.linear(a.cuda()[:37], b.cuda()[:50], ksplit=7, act="relu", bias=torch.ones(50).cuda()).cpu()
    assert rel(out, torch.relu(a[:37] @ b[:50].t() + 1)) < 2e-5
    for T in (4, 5, 3):
        x = torch.randn(7, T, 24, 40, generator=g) * 3
        x[2] = -x[2].abs()                                        # a blank row
        stats, sh, hh = ops.mask_row_stats(x.cuda())
        mn = x[:, ::2] if T >= 5 else x
        soft = F.interpolate(mn, scale_factor=0.5).flatten(1).sigmoid()
        hard = soft.gt(0.5).float()
        assert torch.equal(stats[:, 0].cpu() > 0, x.gt(0).flatten(1).any(1))
        s_full = x.sigmoid().flatten(1); h_full = s_full.gt(0.5).float()
        assert float((stats[:, 1].cpu() - (s_full * h_full).sum(1)).abs().max()) < 2e-2
        assert torch.equal(stats[:, 2].cpu(), h_full.sum(1))
        assert float((sh.cpu() - soft).abs().max()) < 1e-6 and torch.equal(hh.cpu(), hard)
        assert float((stats[:, 3].cpu() - soft.sum(1)).abs().max()) < 2e-2 and torch.equal(stats[:, 4].cpu(), hard.sum(1))


def test_mha_small():
    from mdqe_cvpr2023_amd import ops
    import math
    g = torch.Generator().manual_seed(8)
    for B, Q, C, nh in ((5, 196, 256, 8), (2, 16, 256, 8), (3, 196, 192, 8)):
        qk = torch.randn(B * Q, 2 * C, generator=g) * 2
        v = torch.randn(B * Q, C, generator=g)
        d = C // nh
        q = qk[:, :C].view(B, Q, nh, d).transpose(1, 2)
        k = qk[:, C:].view(B, Q, nh, d).transpose(1, 2)
        vv = v.view(B, Q, nh, d).transpose(1, 2)
        ref = (torch.softmax((q / math.sqrt(d)) @ k.transpose(-1, -2), -1) @ vv).transpose(1, 2).reshape(B * Q, C)
        from mdqe_cvpr2023_amd._lib import lib
        try:
            for variant in (1, 0):                     # fp32-MFMA form and scalar form
                lib.mdqe_debug_mha_variant(variant)
                out = ops.mha_small(qk.cuda(), v.cuda(), B, Q, C, nh).cpu()
                assert float((out - ref).abs().max()) < 2e-5, (B, Q, C, variant)
        finally:
            lib.mdqe_debug_mha_variant(1)


def test_query_select_and_sampling():
    from mdqe_cvpr2023_amd import ops
    import mdqe_oracle as O
    g = torch.Generator().manual_seed(12)
    for (H, W, nb) in ((48, 80, 14), (8, 12, 4), (60, 108, 14)):
        conf = torch.randn(3, H, W, 7, generator=g) * 2
        ref = O.grid_guided_query_selection(conf, nb)
        out = ops.query_select(conf.cuda(), nb).cpu()
        bad = (out - ref).abs().amax(-1) > 1e-6
        assert bad.float().mean() < 0.01                        # argmax may flip only on near-ties
    shapes = [(12, 20), (6, 10), (3, 5), (2, 3)]
    starts = [0, 240, 300, 315]
    tok = torch.randn(2, 321, 64, generator=g)
    coords = torch.rand(2, 16, 2, generator=g)
    coords[0, 0] = torch.tensor([0.0, 0.0]); coords[0, 1] = torch.tensor([0.999, 0.999])
    grid = 2 * coords.view(2, 4, 4, 2) - 1
    acc = 0
    for (Hl, Wl), st in zip(shapes, starts):
        f = tok[:, st:st + Hl * Wl].transpose(1, 2).reshape(2, 64, Hl, Wl)
        acc = acc + F.grid_sample(f, grid, mode="bilinear", padding_mode="border", align_corners=False)
    ref = (acc / 4).flatten(2).transpose(1, 2)
    out = ops.sample_levels_mean(tok.cuda(), coords.cuda(), shapes, starts).cpu()
    assert float((out - ref).abs().max()) < 1e-5


def test_final_masks():
    from mdqe_cvpr2023_amd import ops
    import mdqe_oracle as O
    g = torch.Generator().manual_seed(4)
    lg = torch.randn(5, 3, 16, 24, generator=g) * 2
    h, w, Ho, Wo = 60, 90, 120, 180
    up = O.aligned_bilinear(lg, 4).sigmoid()[..., :h, :w]
    sel = [0, 2, 3]
    ref = torch.stack([F.interpolate(up[i].unsqueeze(0), size=(Ho, Wo), mode="nearest").squeeze(0) > 0.5 for i in sel])
    out = torch.zeros(3, 5, Ho, Wo, dtype=torch.uint8).cuda()
    ops.final_masks(lg.cuda(), torch.tensor(sel, dtype=torch.int32).cuda(), 4, h, w, Ho, Wo, out, 1)
    got = out.cpu().bool()
    assert (got[:, 1:4] != ref).float().mean() < 1e-4
    assert not got[:, 0].any() and not got[:, 4].any()


def test_gemm_f16x3_accuracy():
    """Split-precision GEMM/conv (f16 hi + scaled f16 lo, 3 MFMAs, fp32 accumulate) vs an fp64 reference: the error
    must be of the order of the fp32 MFMA kernel's own error (<= 4x), i.e. ~1e-6 relative."""
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(21)
    try:
        for (M, N, K) in ((20000, 640, 256), (20000, 256, 1024), (3000, 1024, 256)):
            x = torch.randn(M, K, generator=g) * 3
            x[::7] *= 1e-3                                     # small rows: exercises the scaled low part
            w = torch.randn(N, K, generator=g) / K ** 0.5
            b = torch.randn(N, generator=g)
            ref = (x.double() @ w.double().t() + b.double())
            ops.set_gemm_precision("f32")
            e32 = float((ops.linear(x.cuda(), w.cuda(), b.cuda(), tile=1).cpu().double() - ref).abs().max() / ref.abs().max())
            ops.set_gemm_precision("f16x3")
            o3 = ops.linear(x.cuda(), w.cuda(), b.cuda(), tile=1).cpu().double()
            e3 = float((o3 - ref).abs().max() / ref.abs().max())
            assert e3 < max(4 * e32, 2e-6), (M, N, K, e32, e3)
            # per-row relative error on the small-magnitude rows too
            rows = slice(0, M, 7)
            er = float((o3[rows] - ref[rows]).abs().max() / ref[rows].abs().max())
            assert er < 5e-6, er
        # implicit-GEMM conv in split precision
        xi = torch.randn(2, 256, 24, 40, generator=g); wc = torch.randn(256, 256, 3, 3, generator=g) / 48; bc = torch.randn(256, generator=g)
        ref = F.conv2d(xi.double(), wc.double(), bc.double(), 1, 1)
        out = ops.conv2d_nhwc(xi.permute(0, 2, 3, 1).contiguous().cuda(), wc.permute(0, 2, 3, 1).contiguous().cuda(), bc.cuda(), 1, 1, tile=1)
        assert float((out.cpu().permute(0, 3, 1, 2).double() - ref).abs().max() / ref.abs().max()) < 3e-6
    finally:
        ops.set_gemm_precision("f32")


def test_gemm_f16x3_presplit_weights():
    """f16x3 with pre-split constant weights (gemm_f16x3w.hip: 128 x 256 / 128 x 128 tiles, single scaled accumulator) vs
    an fp64 reference and vs the in-kernel-split f16x3 kernel: same accuracy class (<= 4x the fp32 MFMA kernel's error),
    every epilogue option, ragged M / N / K, conv mode with padding and stride."""
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(33)
    try:
        for (M, N, K) in ((20000, 640, 256), (40000, 256, 1024), (33000, 1024, 256), (26001, 3072, 256), (40000, 328, 136)):
            x = torch.randn(M, K, generator=g) * 3
            x[::7] *= 1e-3
            w = torch.randn(N, K, generator=g) / K ** 0.5
            b = torch.randn(N, generator=g)
            ref = (x.double() @ w.double().t() + b.double())
            xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
            ops.set_gemm_precision("f32")
            e32 = float((ops.linear(xd, wd, bd, tile=1).cpu().double() - ref).abs().max() / ref.abs().max())
            ops.set_gemm_precision("f16x3")
            ops.const_weight(wd)
            assert (ops._wsplit(wd) is not None) == (K % 32 == 0)      # ragged K stays on the in-kernel-split kernel
            o3 = ops.linear(xd, wd, bd, tile=1).cpu().double()
            e3 = float((o3 - ref).abs().max() / ref.abs().max())
            assert e3 < max(4 * e32, 2e-6), (M, N, K, e32, e3)
            rows = slice(0, M, 7)
            er = float((o3[rows] - ref[rows]).abs().max() / ref[rows].abs().max())
            assert er < 5e-6, er
        # epilogue: gelu on the first columns, residual broadcast by res_mod, row mask, strided output
        M, N, K = 25600, 640, 256
        x = torch.randn(M, K, generator=g); w = torch.randn(N, K, generator=g) / 16; b = torch.randn(N, generator=g)
        res = torch.randn(5120, N, generator=g); rm = torch.rand(M, generator=g) < 0.2
        wd = ops.const_weight(w.cuda())
        out = torch.full((M, N + 64), 7.0, device="cuda")
        ops.linear(x.cuda(), wd, b.cuda(), act="gelu", act_cols=256, residual=res.cuda(), res_mod=5120, rowmask=rm.cuda(), mask_cols=256,
                   out=out, ldc=N + 64, tile=1)
        y = x.double() @ w.double().t() + b.double()
        y[:, :256] = F.gelu(y[:, :256])
        y = y + res.double().repeat(M // 5120, 1)
        y[:, :256][rm] = 0
        assert float((out[:, :N].cpu().double() - y).abs().max()) < 2e-5
        assert bool((out[:, N:] == 7.0).all())
        # in-place update of the weight invalidates the planes (falls back to the in-kernel split, still correct)
        wd.mul_(2.0)
        assert ops._wsplit(wd) is None
        o = ops.linear(x.cuda(), wd, b.cuda(), tile=1).cpu().double()
        yy = x.double() @ (2 * w.double()).t() + b.double()
        assert float((o - yy).abs().max() / yy.abs().max()) < 3e-6
        # implicit-GEMM conv: 3x3 pad 1, 3x3 stride 2, 1x1, with residual-before-relu
        for (Cin, Cout, k, s, p_) in ((256, 256, 3, 1, 1), (512, 512, 3, 2, 1), (1024, 256, 1, 1, 0)):
            xi = torch.randn(6, Cin, 24, 40, generator=g); wc = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
            bc = torch.randn(Cout, generator=g)
            ref = F.conv2d(xi.double(), wc.double(), bc.double(), s, p_)
            rs = torch.randn(ref.shape, generator=g)
            ref = F.relu(ref + rs.double())
            wk = ops.const_weight(wc.permute(0, 2, 3, 1).contiguous().cuda())
            assert ops._wsplit(wk) is not None
            out = ops.conv2d_nhwc(xi.permute(0, 2, 3, 1).contiguous().cuda(), wk, bc.cuda(), s, p_, act="relu",
                                  residual=rs.permute(0, 2, 3, 1).contiguous().cuda(), res_first=True, tile=1)
            assert float((out.cpu().permute(0, 3, 1, 2).double() - ref).abs().max() / ref.abs().max()) < 3e-6, (Cin, Cout, k, s)
    finally:
        ops.set_gemm_precision("f32")


@pytest.mark.parametrize("N,nh,nW,shifted", [(144, 6, 12, True), (144, 3, 1, False), (36, 4, 6, True), (64, 2, 1, False)])
def test_window_attention_mfma_vs_fp64_and_scalar_form(N, nh, nW, shifted):
    """Cosine window attention (swin_transformer_v2.py:147-186) on the fp32 matrix cores vs an fp64 evaluation of the same
    formula and vs the scalar kernel form."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import lib
    g = torch.Generator().manual_seed(41)
    C, nwin = 32 * nh, 2 * nW + 1
    qkv = torch.randn(nwin * N, 3 * C, generator=g)
    scale = torch.rand(nh, generator=g) * 20 + 1
    bias = torch.randn(nh, N, N, generator=g)
    mask = None
    if shifted:
        mask = torch.where(torch.rand(nW, N, N, generator=g) < 0.3, torch.tensor(-100.0), torch.tensor(0.0))
    q, k, v = (qkv[:, i * C:(i + 1) * C].double().view(nwin, N, nh, 32).transpose(1, 2) for i in range(3))
    att = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-1, -2) * scale.double().view(1, nh, 1, 1) + bias.double()[None]
    if mask is not None:
        att = att + mask.double()[torch.arange(nwin) % nW][:, None]
    ref = (att.softmax(-1) @ v).transpose(1, 2).reshape(nwin * N, C)
    outs = []
    try:
        for variant in (1, 0):
            lib.mdqe_debug_window_attn_variant(variant)
            outs.append(ops.window_attn(qkv.cuda(), nwin, N, C, nh, scale.cuda(), bias.cuda(), None if mask is None else mask.cuda(), nW).cpu())
    finally:
        lib.mdqe_debug_window_attn_variant(1)
    for o in outs:
        assert float((o.double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))
    assert float((outs[0] - outs[1]).abs().max()) < 2e-5


@pytest.mark.parametrize("shape", [(72, 128, 36, 64), (75, 133, 36, 64), (50, 80, 100, 160), (97, 61, 33, 20), (40, 40, 40, 57),
                                   (123, 77, 123, 30), (720, 1280, 360, 640), (480, 853, 360, 640)])
def test_device_resize_is_bit_identical_to_the_pillow_restatement(shape):
    """preprocess.resize_frames (HIP) vs oracle/resize_oracle.py, which tests/test_resize_cpu.py pins to PIL bit for bit."""
    import numpy as np
    import resize_oracle as RO
    from mdqe_cvpr2023_amd import preprocess as P
    h, w, oh, ow = shape
    rng = np.random.RandomState(h + w)
    imgs = rng.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    dev = torch.from_numpy(imgs).permute(0, 3, 1, 2).contiguous().cuda()
    got = P.resize_frames(dev, oh, ow).cpu().permute(0, 2, 3, 1).numpy()
    for i in range(2):
        assert np.array_equal(got[i], RO.resize_bilinear_u8(imgs[i], oh, ow)), (shape, i)


def test_conv_splitk_deep_k_few_pixels():
    """input_proj's 3x3 / stride-2 conv on res5 (K = 18432, a few thousand output pixels): split-K spreads it over the CUs;
    same result as the single-pass kernel (fixed summation order per chunk) and as fp64 within fp32 noise."""
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(13)
    xi = torch.randn(6, 2048, 12, 20, generator=g); wc = torch.randn(256, 2048, 3, 3, generator=g) / 136; bc = torch.randn(256, generator=g)
    ref = F.conv2d(xi.double(), wc.double(), bc.double(), 2, 1)
    x, w = xi.permute(0, 2, 3, 1).contiguous().cuda(), wc.permute(0, 2, 3, 1).contiguous().cuda()
    a = ops.conv2d_nhwc(x, w, bc.cuda(), 2, 1, ksplit=1).cpu().permute(0, 3, 1, 2).double()
    b = ops.conv2d_nhwc(x, w, bc.cuda(), 2, 1).cpu().permute(0, 3, 1, 2).double()          # auto: split-K
    c = ops.conv2d_nhwc(x, w, bc.cuda(), 2, 1, act="relu", ksplit=5).cpu().permute(0, 3, 1, 2).double()
    s = float(ref.abs().max())
    tol = 1e-5 * s                                     # an fp32 chain of 18432 terms
    assert float((a - ref).abs().max()) < tol and float((b - ref).abs().max()) < tol
    assert float((c - F.relu(ref)).abs().max()) < tol
    assert float((a - b).abs().max()) < tol


def test_linear_layernorm_fused():
    """mdqe_gemm_ln_f32: LN(x W^T + b + residual) in the GEMM epilogue (64x256 tile) against torch fp32; ragged row count,
    output aliasing the residual, both K of the encoder (256 attention out-proj, 1024 FFN)."""
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(21)
    for M, K in ((16384 + 37, 256), (20000, 1024)):
        x = torch.randn(M, K, generator=g); w = torch.randn(256, K, generator=g) / K ** 0.5; b = torch.randn(256, generator=g)
        r = torch.randn(M, 256, generator=g) * 3 + 0.5
        ga = torch.randn(256, generator=g); be = torch.randn(256, generator=g)
        ref = F.layer_norm(x.double() @ w.double().t() + b.double() + r.double(), (256,), ga.double(), be.double(), 1e-5).float()
        rc = r.cuda()
        out = ops.linear_ln(x.cuda(), w.cuda(), b.cuda(), rc, ga.cuda(), be.cuda())
        assert float((out.cpu() - ref).abs().max()) < 2e-5
        two = ops.layernorm(ops.linear(x.cuda(), w.cuda(), b.cuda(), residual=rc), ga.cuda(), be.cuda())
        assert float((out - two).abs().max()) < 1e-5
        out2 = ops.linear_ln(x.cuda(), w.cuda(), b.cuda(), rc, ga.cuda(), be.cuda(), out=rc)      # in place over the residual
        assert out2.data_ptr() == rc.data_ptr() and torch.equal(out2, out)


def test_linear_layernorm_never_touches_rows_past_m():
    """The LayerNorm epilogue stores through buffer resources whose scalar offset carries the row group: with a ragged M the last tile's
    groups past row M must not be written (or read) at all -- the engine passes `out=x2`, ring views and C2 buffers whose neighbours are
    live tensors.  out, residual and C2 are `[:M]` views of larger canary-filled buffers, M % 64 in {1, 27, 37, 63}: the canary rows
    behind M stay bit for bit what they were, rows below M equal the launch on exact-size tensors."""
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator(device="cuda").manual_seed(77)
    CANARY = 12345.678
    for M, K in ((16384 + 27, 256), (16384 + 37, 1024), (16384 * 2 + 1, 256), (16384 + 63, 256)):
        pad = 192                                              # three tiles of canary rows behind M
        x = torch.randn(M, K, device="cuda", generator=g); w = torch.randn(256, K, device="cuda", generator=g) / K ** 0.5
        b = torch.randn(256, device="cuda", generator=g)
        g1, b1 = torch.randn(256, device="cuda", generator=g), torch.randn(256, device="cuda", generator=g)
        g2, b2 = torch.rand(256, device="cuda", generator=g) + 0.5, torch.randn(256, device="cuda", generator=g)
        r_exact = torch.randn(M, 256, device="cuda", generator=g)
        want1, want2 = ops.linear_ln(x, w, b, r_exact.clone(), g1, b1, second=(g2, b2))
        for second in (None, (g2, b2)):
            big_r = torch.full((M + pad, 256), CANARY, device="cuda"); big_r[:M] = r_exact
            big_o = torch.full((M + pad, 256), CANARY, device="cuda")
            res = ops.linear_ln(x, w, b, big_r[:M], g1, b1, out=big_o[:M], second=second)
            o1 = res if second is None else res[0]
            assert torch.equal(o1, want1) and bool((big_o[M:] == CANARY).all()) and bool((big_r[M:] == CANARY).all()), (M, K, second is not None)
            if second is not None:
                assert torch.equal(res[1], want2)
            # in place over the residual view (the encoder's `out=x2`)
            res = ops.linear_ln(x, w, b, big_r[:M], g1, b1, out=big_r[:M], second=second)
            o1 = res if second is None else res[0]
            assert torch.equal(o1, want1) and bool((big_r[M:] == CANARY).all()), (M, K, "in place")
    # C2 as a view of a canary buffer: through the C ABI (ops.linear_ln allocates C2 itself)
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    M, K = 16384 + 27, 256
    x = torch.randn(M, K, device="cuda", generator=g); w = torch.randn(256, K, device="cuda", generator=g) / K ** 0.5
    b = torch.randn(256, device="cuda", generator=g); r = torch.randn(M, 256, device="cuda", generator=g)
    want1, want2 = ops.linear_ln(x, w, b, r.clone(), g1, b1, second=(g2, b2))
    big_o = torch.full((M + 192, 256), CANARY, device="cuda"); big_2 = torch.full((M + 192, 256), CANARY, device="cuda")
    check(lib.mdqe_gemm_ln2_f32(ptr(x), K, ptr(w), ptr(b), ptr(big_o), 256, M, 256, K, ptr(r), 256, ptr(g1), ptr(b1), ptr(g2), ptr(b2),
                                ptr(big_2), 256, 1e-5, cur_stream()), "gemm_ln2_f32")
    assert torch.equal(big_o[:M], want1) and torch.equal(big_2[:M], want2)
    assert bool((big_o[M:] == CANARY).all()) and bool((big_2[M:] == CANARY).all())


def test_linear_layernorm_with_a_second_layernorm_in_the_epilogue():
    """mdqe_gemm_ln2_f32 (round 4): `x = norm3(x + ffn(x))` and the shared `decoder_norm(x)` that feeds the box head
    (transformer_dec.py:352-358,492-495) from ONE epilogue.  The first output equals mdqe_gemm_ln_f32's and the second equals
    mdqe_layernorm_f32 applied to the first, BIT FOR BIT (same reduction tree) -- so which form a launch takes (one-kernel form from
    16384 rows up, GEMM + two LayerNorm launches below) never changes a result; ragged row counts, both K of the decoder."""
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    for M, K in ((29008, 1024), (16384 + 37, 256), (204000, 1024), (7252, 1024)):
        x = torch.randn(M, K, device="cuda", generator=g); w = torch.randn(256, K, device="cuda", generator=g) / K ** 0.5
        b = torch.randn(256, device="cuda", generator=g); r = torch.randn(M, 256, device="cuda", generator=g) * 3 + 0.5
        g1, b1 = torch.randn(256, device="cuda", generator=g), torch.randn(256, device="cuda", generator=g)
        g2, b2 = torch.rand(256, device="cuda", generator=g) + 0.5, torch.randn(256, device="cuda", generator=g)
        one = ops.linear_ln(x, w, b, r, g1, b1)
        want2 = ops.layernorm(one, g2, b2)
        got1, got2 = ops.linear_ln(x, w, b, r, g1, b1, second=(g2, b2))
        assert torch.equal(got1, one) and torch.equal(got2, want2), (M, K)
        old = ops.LINEAR_LN2_FUSED
        try:
            ops.LINEAR_LN2_FUSED = False               # the second LayerNorm as its own launch
            a1, a2 = ops.linear_ln(x, w, b, r, g1, b1, second=(g2, b2))
        finally:
            ops.LINEAR_LN2_FUSED = old
        assert torch.equal(a1, one) and torch.equal(a2, want2)
    ref = F.layer_norm(F.layer_norm(x.double() @ w.double().t() + b.double() + r.double(), (256,), g1.double(), b1.double(), 1e-5),
                       (256,), g2.double(), b2.double(), 1e-5)
    assert float((got2.double() - ref).abs().max()) < 3e-5


@pytest.mark.parametrize("shapes,B,M,D", [
    ([(12, 20), (6, 10), (3, 5), (2, 3)], 3, 8, 32),          # 96x160 frames
    ([(8, 12), (4, 6), (2, 3), (1, 2)], 17, 8, 32),           # the tests' 64x96 frames; 17 >= 16 frames: XCD-aware block order
    ([(48, 80), (24, 40), (12, 20), (6, 10)], 2, 8, 32),      # R50_ovis_360 (two coarse levels staged, 38 KB)
    ([(15, 27), (8, 14), (4, 7), (2, 4)], 2, 8, 24),          # Swin-L's head width
    ([(80, 144), (40, 72), (20, 36), (10, 18)], 1, 8, 32),    # R50_ovis_720 (115 KB staged, 512 queries per block)
])
def test_encoder_msda_with_coarse_levels_in_lds_equals_the_gather_form(shapes, B, M, D):
    """msda_fused_v3_kernel (coarse levels staged in LDS per (frame, head)) against msda_fused_v2_kernel (every corner through the
    texture path), which the reference goldens hold to the reference: same lane mapping and order of operations -> equal bits;
    locations from inside the maps to far outside them, and onto pixel borders."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import lib
    g = torch.Generator().manual_seed(B * 7 + D)
    L, P = 4, 4
    C = M * D
    Nq = sum(h * w for h, w in shapes)
    starts = [0]
    for h, w in shapes[:-1]:
        starts.append(starts[-1] + h * w)
    levels = ([s[0] for s in shapes], [s[1] for s in shapes], starts)
    nq = 2 * M * L * P
    proj = torch.randn(B * Nq, C + 3 * M * L * P, generator=g)
    proj[:, C:C + nq] *= 3.0                                                  # offsets up to ~ +-1.5 maps
    proj[::7, C:C + nq] = torch.round(proj[::7, C:C + nq])                    # exact eighths -> pixel borders on the /8 levels
    proj = proj.cuda()
    ref = torch.cat([torch.stack(torch.meshgrid((torch.arange(a) + 0.5) / a, (torch.arange(c) + 0.5) / c, indexing="ij"), -1).reshape(-1, 2).flip(-1)
                     for a, c in shapes]).float().cuda().contiguous()
    outs = []
    try:
        for var in (1, 9):
            lib.mdqe_debug_msda_variant(var)
            out = torch.full((B * Nq, C), float("nan"), device="cuda")
            ops.msda_fused(proj[:, :C], proj[:, C:C + nq], proj[:, C + nq:], ref, levels, B, Nq, M, D, L, P, mode=0, v_brows=Nq, out=out)
            outs.append(out)
        # round 6's experiment (off by default, measured slower): a block iteration as an 8 x 16 patch of queries -- every output row, patches
        # over the levels' edges included (NaN-filled output: a row a patch skipped would show)
        lib.mdqe_debug_msda_variant(9)
        lib.mdqe_debug_msda_patch(1)
        out = torch.full((B * Nq, C), float("nan"), device="cuda")
        ops.msda_fused(proj[:, :C], proj[:, C:C + nq], proj[:, C + nq:], ref, levels, B, Nq, M, D, L, P, mode=0, v_brows=Nq, out=out)
        outs.append(out)
    finally:
        lib.mdqe_debug_msda_variant(-1)
        lib.mdqe_debug_msda_patch(0)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("Q,BT", [(196, 9), (64, 20), (300, 3)])
def test_decoder_box_level_msda_with_coarse_levels_in_lds_equals_the_gather_form(Q, BT):
    """The decoder's box-level launch (mode 1: grid pattern scaled by the query's box + clamped delta, value block picked per batch
    element) on msda_fused_v3_kernel against msda_fused_v2_kernel: equal bits; Q = 196 runs as two runs of 98 queries on 13 waves."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import lib
    g = torch.Generator().manual_seed(Q)
    M, D, L, P, F = 8, 32, 4, 4, 6
    shapes = [(12, 20), (6, 10), (3, 5), (2, 3)]
    N = sum(h * w for h, w in shapes)
    starts = [0]
    for h, w in shapes[:-1]:
        starts.append(starts[-1] + h * w)
    levels = ([s[0] for s in shapes], [s[1] for s in shapes], starts)
    wide = torch.randn(F * N, 3 * 256, generator=g).cuda()
    nq = 2 * M * L * P
    pr = (2.0 * torch.randn(BT * Q, 3 * M * L * P, generator=g)).cuda()
    boxes = (torch.rand(BT, Q, 4, generator=g) * torch.tensor([1, 1, 0.5, 0.5])).cuda()
    grid = torch.randn(M * L * P * 2, generator=g).cuda()
    vidx = torch.randint(0, F, (BT,), generator=g, dtype=torch.int32).cuda()
    outs = []
    try:
        for var in (0, 8):
            lib.mdqe_debug_msda_variant(var)
            out = torch.full((BT * Q, 256), float("nan"), device="cuda")
            ops.msda_fused(wide[:, 256:512], pr[:, :nq], pr[:, nq:], boxes, levels, BT, Q, M, D, L, P, mode=1, grid=grid, v_brows=N, vidx=vidx, out=out)
            outs.append(out)
    finally:
        lib.mdqe_debug_msda_variant(-1)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_fused_msda_on_a_value_cache_larger_than_4_gb():
    """The decoder reads its value maps as 256-column slices of the [frames x tokens, 3072] cache, which passes 4 GB at 640p (or with
    60-frame passes at 360p).  The gather kernels address with 32-bit buffer offsets: their resource is based at the ELEMENT's block, so
    only one element's levels must fit the offset range.  Same launch on the big cache and on a compact copy of the frames it reads:
    equal bits (box-level form on the staged kernel, temporal form -- 4 frames per element -- on v2)."""
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    M, D, L, P, Q = 8, 32, 4, 4, 196
    shapes = [(48, 80), (24, 40), (12, 20), (6, 10)]
    N = sum(h * w for h, w in shapes)
    starts = [0]
    for h, w in shapes[:-1]:
        starts.append(starts[-1] + h * w)
    F = 72                                                         # 72 x 5100 rows x 3072 columns x 4 B = 4.5 GB
    wide = torch.randn(F * N, 3072, device="cuda", generator=g)
    assert wide.numel() * 4 > 2 ** 32
    frames = [70, 3, 71, 68]                                       # blocks beyond the 4-GB mark and before it
    compact = torch.cat([wide[f * N:(f + 1) * N] for f in frames + [69]]).contiguous()     # (+ frame 69: the temporal form reads 68..71)
    nq = 2 * M * L * P
    pr = 2.0 * torch.randn(len(frames) * Q, 3 * M * L * P, device="cuda", generator=g)
    boxes = torch.rand(len(frames), Q, 4, device="cuda", generator=g) * torch.tensor([1, 1, 0.5, 0.5], device="cuda")
    grid = torch.randn(M * L * P * 2, device="cuda", generator=g)
    lv = ([s[0] for s in shapes], [s[1] for s in shapes], starts)
    col = slice(1024, 1280)
    outs = []
    for buf, vidx in ((wide, frames), (compact, [0, 1, 2, 3])):
        out = torch.empty(len(frames) * Q, 256, device="cuda")
        ops.msda_fused(buf[:, col], pr[:, :nq], pr[:, nq:], boxes, lv, len(frames), Q, M, D, L, P, mode=1, grid=grid, v_brows=N,
                       vidx=torch.tensor(vidx, dtype=torch.int32, device="cuda"), out=out)
        outs.append(out)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    # temporal form: one element = 4 consecutive frames (68..71 of the big cache = rows 3, 4, 2(71)... of the compact copy do not line up,
    # so the compact copy is rebuilt in frame order)
    compact_t = wide[68 * N:72 * N].contiguous()
    Tc = 4
    lv_tp = ([s[0] for s in shapes for _ in range(Tc)], [s[1] for s in shapes for _ in range(Tc)], [f * N + starts[gi] for gi in range(L) for f in range(Tc)])
    pr_t = pr[:Q]
    ib = boxes[:1]
    outs = []
    for buf, first in ((wide, 68), (compact_t, 0)):
        out = torch.empty(Q, 256, device="cuda")
        ops.msda_fused(buf[:, col], pr_t[:, :nq], pr_t[:, nq:], ib, lv_tp, 1, Q, M, D, Tc, P, mode=1, grid=grid, groups=L, scale=0.25, v_brows=N,
                       vidx=torch.tensor([first], dtype=torch.int32, device="cuda"), out=out)
        outs.append(out)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("M,N,K,act", [(31360, 4, 256, None), (31361, 1, 256, None), (2050, 8, 512, "sigmoid"), (7843, 3, 256, "relu")])
def test_linear_with_a_few_output_columns(M, N, K, act):
    """rows_dot_kernel (N <= 8: the decoder's box head and time weights) against fp64, and against the MFMA tiles it replaces."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import lib
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K + 64, generator=g).cuda()[:, :K]                     # a padded row pitch
    w, b = (torch.randn(N, K, generator=g) / 16).cuda(), torch.randn(N, generator=g).cuda()
    ref = x.double() @ w.double().t() + b.double()
    if act == "sigmoid":
        ref = torch.sigmoid(ref)
    elif act == "relu":
        ref = torch.relu(ref)
    out = ops.linear(x, w, b, act=act)
    try:
        lib.mdqe_debug_gemm_rows_dot(0)
        out_mfma = ops.linear(x, w, b, act=act)
    finally:
        lib.mdqe_debug_gemm_rows_dot(1)
    scale = float(ref.abs().max())
    assert float((out.double() - ref).abs().max()) < 2e-6 * max(scale, 1.0)
    assert float((out - out_mfma).abs().max()) < 4e-6 * max(scale, 1.0)


@pytest.mark.parametrize("NI,H2,W2,K2,K1,N,stride", [(3, 24, 40, 64, 64, 256, 1), (2, 24, 40, 256, 128, 512, 2), (5, 13, 21, 512, 256, 1024, 2),
                                                    (1, 7, 9, 1024, 512, 2048, 2), (40, 12, 20, 64, 64, 256, 1)])
def test_bottleneck_conv3_and_projection_shortcut_as_one_product(NI, H2, W2, K2, K1, N, stride):
    """mdqe_gemm_nt_cat2_f32 (second A operand = the block's input read with the shortcut's stride) against the two-launch form it
    replaces and against fp64; odd map sizes (13 x 21 -> 7 x 11 at stride 2)."""
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(N + NI)
    OH, OW = (H2 - 1) // stride + 1, (W2 - 1) // stride + 1
    x = torch.randn(NI, H2, W2, K2, generator=g).cuda()
    y = torch.randn(NI, OH, OW, K1, generator=g).cuda()
    w3, ws = (torch.randn(N, K1, generator=g) / K1 ** 0.5).cuda(), (torch.randn(N, K2, generator=g) / K2 ** 0.5).cuda()
    b3, bs = torch.randn(N, generator=g).cuda(), torch.randn(N, generator=g).cuda()
    out = ops.linear_cat2(y, x, stride, torch.cat([w3, ws], 1).contiguous(), b3 + bs, act="relu")
    xs = x[:, ::stride, ::stride].contiguous()
    ref = torch.relu(y.double().reshape(-1, K1) @ w3.double().t() + xs.double().reshape(-1, K2) @ ws.double().t() + (b3 + bs).double()).view(NI, OH, OW, N)
    sc = ops.conv2d_nhwc(x, ws.view(N, 1, 1, K2), bs, stride, 0)
    two = ops.linear(y.view(-1, K1), w3, b3, act="relu", residual=sc.view(-1, N), res_first=True).view(NI, OH, OW, N)
    scale = float(ref.abs().max())
    assert float((out.double() - ref).abs().max()) < 3e-6 * scale
    assert float((out - two).abs().max()) < 6e-6 * scale


@pytest.mark.parametrize("shapes,D,Tclip", [([(48, 80), (24, 40), (12, 20), (6, 10)], 32, 4), ([(60, 108), (30, 54), (15, 27), (8, 14)], 24, 4),
                                             ([(80, 144), (40, 72), (20, 36), (10, 18)], 32, 3)])
def test_temporal_msda_kernel_vs_the_oracle_at_full_size(shapes, D, Tclip):
    """msda_fused_tp_kernel held DIRECTLY to the oracle's restatement of MSDeformAttn.temporal_clip_forward (ms_deform_attn.py:175-238 ->
    oracle.msda_temporal, evaluated in float64) at the full 360p / Swin-L / 640p level tables -- until round 4 its only oracle-level
    check went through the reduced decoder goldens.  The module's linears are made identities / selections, so the oracle consumes exactly
    the offsets, logits and value maps the kernel consumes; Tclip = 3: a short clip, whose last frame is repeated (transformer_dec.py:382-386)."""
    import mdqe_oracle as O
    from mdqe_cvpr2023_amd import ops
    from _golden import record_margin
    g = torch.Generator().manual_seed(11 + D)
    M, L, P, Tc, Q, Bc = 8, 4, 4, 4, 196, 2
    C = M * D
    N = sum(h * w for h, w in shapes)
    starts = [0]
    for h, w in shapes[:-1]:
        starts.append(starts[-1] + h * w)
    Fr = Bc + Tclip - 1
    vals = torch.randn(Fr, N, C, generator=g)
    off = 2.0 * torch.randn(Bc, Q, 2 * M * Tc * P, generator=g)
    lg = 2.0 * torch.randn(Bc, Q, M * Tc * P, generator=g)
    ibox = torch.rand(Bc, Q, 4, generator=g) * torch.tensor([1, 1, 0.6, 0.6])
    ibox[0, :5, :2] = torch.tensor([0.0, 1.0])
    grid = O.msda_dir_grid(M, Tc, P)                                   # the module's fixed buffer [M, Tc, P, 2]
    tca = list(range(Tclip)) + [Tclip - 1] * (Tc - Tclip)             # frames the Tc slots read (last frame repeated)
    lv_tp = ([s[0] for s in shapes for _ in range(Tc)], [s[1] for s in shapes for _ in range(Tc)], [f * N + starts[gi] for gi in range(L) for f in tca])
    nq = 2 * M * Tc * P
    pr = torch.cat([off, lg], -1).reshape(Bc * Q, -1).cuda()
    out = torch.full((Bc * Q, C), float("nan"), device="cuda")
    ops.msda_fused(vals.reshape(Fr * N, C).cuda(), pr[:, :nq], pr[:, nq:], ibox.cuda(), lv_tp, Bc, Q, M, D, Tc, P, mode=1,
                   grid=grid.reshape(-1).cuda().contiguous(), groups=L, scale=1.0 / L, v_brows=N,
                   vidx=torch.arange(Bc, dtype=torch.int32).cuda(), out=out)
    # the oracle's module with identity value / output projections and selection matrices for the two query projections
    K = 3 * M * Tc * P
    eye = torch.eye(C, dtype=torch.float64)
    sd = {"m.value_proj.weight": eye, "m.value_proj.bias": torch.zeros(C, dtype=torch.float64), "m.output_proj.weight": eye,
          "m.output_proj.bias": torch.zeros(C, dtype=torch.float64), "m.sampling_offsets": grid.double(),
          "m.sampling_grid_offsets.weight": torch.eye(K, dtype=torch.float64)[:nq], "m.sampling_grid_offsets.bias": torch.zeros(nq, dtype=torch.float64),
          "m.attention_weights.weight": torch.eye(K, dtype=torch.float64)[nq:], "m.attention_weights.bias": torch.zeros(K - nq, dtype=torch.float64)}
    worst = 0.0
    for b in range(Bc):
        x = torch.stack([vals[b + t] for t in tca]).double()[None]                  # [1, Tc, N, C]
        q = torch.cat([off[b], lg[b]], -1).double()[None]                           # [1, Q, K]
        ref = O.msda_temporal(sd, "m", q, ibox[b].double()[None], x, shapes, None, M, P, Tc)[0]
        got = out.view(Bc, Q, C)[b].cpu().double()
        worst = max(worst, float((got - ref).abs().max()) / max(1.0, float(ref.abs().max())))
    record_margin("kernels vs the float64 oracle, full-size level tables", "temporal MSDA (msda_fused_tp_kernel) D=%d T=%d %dx%d" % (D, Tclip, *shapes[0]), worst, 1.0, 1e-5)
    assert worst < 1e-5


@pytest.mark.parametrize("shapes,D,Q,Bc", [([(48, 80), (24, 40), (12, 20), (6, 10)], 32, 196, 37), ([(12, 20), (6, 10), (3, 5), (2, 3)], 32, 49, 5),
                                            ([(60, 108), (30, 54), (15, 27), (8, 14)], 24, 196, 6), ([(80, 144), (40, 72), (20, 36), (10, 18)], 32, 196, 3)])
def test_temporal_msda_with_frame_by_frame_staging_equals_the_gather_form(shapes, D, Q, Bc):
    """The decoder's instance-level launch (every (clip, query, head): 4 frames x 4 points, each on all 4 levels of its frame, averaged):
    msda_fused_tp_kernel -- the block walks the frames, staging each frame's coarse levels in LDS -- against msda_fused_v2_kernel (every
    corner through the texture path).  Frame-major instead of level-major summation: 1e-5 of the output scale.  360p / small / Swin-L
    (D = 24) / 640p level tables (the last two stage the coarsest level only)."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import lib
    g = torch.Generator(device="cuda").manual_seed(Q + D)
    M, L, P, Tc = 8, 4, 4, 4
    C = M * D
    N = sum(h * w for h, w in shapes)
    starts = [0]
    for h, w in shapes[:-1]:
        starts.append(starts[-1] + h * w)
    Fr = Bc + Tc - 1
    vals = torch.randn(Fr * N, C, device="cuda", generator=g)
    nq = 2 * M * Tc * P
    pr = 2.0 * torch.randn(Bc * Q, 3 * M * Tc * P, device="cuda", generator=g)
    ibox = torch.rand(Bc, Q, 4, device="cuda", generator=g) * torch.tensor([1, 1, 0.6, 0.6], device="cuda")
    ibox[0, :5, :2] = torch.tensor([0.0, 1.0], device="cuda")                     # boxes on the frame's corners: corners outside the maps
    grid = torch.randn(M * Tc * P * 2, device="cuda", generator=g)
    lv_tp = ([s[0] for s in shapes for _ in range(Tc)], [s[1] for s in shapes for _ in range(Tc)], [f * N + starts[gi] for gi in range(L) for f in range(Tc)])
    vidx = torch.arange(Bc, dtype=torch.int32, device="cuda")
    outs = []
    try:
        for staged in (1, 0):
            lib.mdqe_debug_msda_tp_staged(staged)
            out = torch.full((Bc * Q, C), float("nan"), device="cuda")
            ops.msda_fused(vals, pr[:, :nq], pr[:, nq:], ibox, lv_tp, Bc, Q, M, D, Tc, P, mode=1, grid=grid, groups=L, scale=0.25, v_brows=N, vidx=vidx, out=out)
            outs.append(out)
    finally:
        lib.mdqe_debug_msda_tp_staged(1)
    assert torch.isfinite(outs[0]).all() and not torch.equal(outs[0], torch.zeros_like(outs[0]))
    assert float((outs[0] - outs[1]).abs().max()) <= 1e-5 * float(outs[1].abs().max())


def test_gemm_fast_and_general_epilogue_give_equal_bits():
    """The K-step-16 GEMM sends interior tiles through a few-instruction epilogue and edge tiles / waves with masked rows through the
    general one IN THE SAME LAUNCH: any difference between the two would make a frame's bits depend on the pass it shares (the sharded
    bench's self-verification caught a 1-ulp GELU contraction difference in round 4).  Every form the fast path takes, on against off."""
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gemm_epilogue_paths.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "0 differing cases" in r.stdout


def test_gemm_single_pass_f16_mode():
    """Mode "f16" (round 5; the reference's fp16-autocast arithmetic, train_net.py:207): ONE f16 MFMA pass on the products whose constant
    weight has planes -- operands rounded to nearest f16, fp32 accumulation, fp32 result.  Against float64 the error is that of the two
    roundings (2^-11 relative per operand: ~1e-3 of the output scale at most, far above f16x3's 1e-6 and fp32's 1e-7); it equals the product
    of the ROUNDED operands to fp32 accuracy (the mode really is one f16 pass with exact accumulation); products without planes, or too
    small for the 128-row tile, stay exact fp32; GEMM and implicit-GEMM conv, with the fused epilogue."""
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(31)
    try:
        for (M, N, K) in ((40000, 256, 256), (30000, 1024, 256), (25000, 640, 1024)):
            x = torch.randn(M, K, generator=g).cuda(); w = ops.const_weight((torch.randn(N, K, generator=g) / K ** 0.5).cuda()); b = torch.randn(N, generator=g).cuda()
            r = torch.randn(M, N, generator=g).cuda()
            ops.set_gemm_precision("f32")
            exact = ops.linear(x, w, b, act="gelu", residual=r)
            ops.set_gemm_precision("f16")
            got = ops.linear(x, w, b, act="gelu", residual=r)
            ref = F.gelu(x.double() @ w.double().t() + b.double()) + r.double()
            rounded = F.gelu(x.half().double() @ w.half().double().t() + b.double()) + r.double()
            scale = float(ref.abs().max())
            e64, e_rounded, e32 = float((got.double() - ref).abs().max()) / scale, float((got.double() - rounded).abs().max()) / scale, float((exact.double() - ref).abs().max()) / scale
            assert e32 < 2e-6 and 1e-5 < e64 < 2e-3 and e_rounded < 5e-6, (M, N, K, e32, e64, e_rounded)
        # a weight without planes (N < 128) and a product below the tile rule stay exact fp32 in this mode
        x = torch.randn(30000, 256, generator=g).cuda(); w = (torch.randn(64, 256, generator=g) / 16).cuda()
        ops.set_gemm_precision("f32"); a = ops.linear(x, w)
        ops.set_gemm_precision("f16"); c = ops.linear(x, w)
        assert torch.equal(a, c)
        # implicit-GEMM conv
        xi = torch.randn(8, 48, 80, 128, generator=g).cuda(); wc = ops.const_weight((torch.randn(256, 3, 3, 128, generator=g) / 34).cuda()); bc = torch.randn(256, generator=g).cuda()
        ops.set_gemm_precision("f16")
        got = ops.conv2d_nhwc(xi, wc, bc, 1, 1, act="relu")
        ref = F.relu(F.conv2d(xi.permute(0, 3, 1, 2).half().double(), wc.permute(0, 3, 1, 2).half().double(), bc.double(), 1, 1)).permute(0, 2, 3, 1)
        assert float((got.double() - ref).abs().max()) / float(ref.abs().max()) < 5e-6
    finally:
        ops.set_gemm_precision("f32")
