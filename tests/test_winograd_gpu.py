"""GPU: stride-1 3x3 convolutions as fp32 Winograd F(2x2,3x3) (csrc/winograd.hip, ops.winograd_weight / ops.conv2d_nhwc).
Accuracy against fp64 at the shipped layer shapes (with the direct kernel's error on the same data as the yardstick), frame
independence across the image groups, determinism, and the routing rules (split-precision modes and unregistered weights stay on
the direct implicit GEMM)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _data(NI, H, W, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(NI, H, W, Cin, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g)
    return x, w, b


def _ref64(x, w, b, act):
    y = F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), b.double(), 1, 1).permute(0, 2, 3, 1)
    return F.relu(y) if act == "relu" else y


def _pair(w):
    """(registered weight, an unregistered copy) on the GPU."""
    from mdqe_cvpr2023_amd import ops
    wr = ops.winograd_weight(w.cuda().contiguous())
    wd = w.cuda().contiguous()
    assert ops._wino_u(wr) is not None and ops._wino_u(wd) is None
    return wr, wd


# (NI, H, W, Cin, Cout, act, bias): ResNet-50 360p (res3 / res4 / res5 conv2, mask head lay1-3), 640p (20x36, 40x72, 80x144), Swin-L 480p
# mask head (15x27, 30x54, 60x108) -- odd sizes included
SHAPES = [
    (2, 45, 80, 128, 128, "relu", True),
    (3, 23, 40, 256, 256, "relu", True),
    (4, 12, 20, 512, 512, "relu", True),
    (4, 12, 20, 256, 256, None, True),
    (2, 23, 40, 256, 256, None, True),
    (1, 45, 80, 256, 256, None, True),
    (2, 20, 36, 256, 256, None, True),
    (1, 40, 72, 256, 256, "relu", True),
    (1, 80, 144, 128, 128, "relu", False),
    (2, 15, 27, 256, 256, None, True),
    (1, 30, 54, 256, 256, None, False),
    (1, 60, 108, 256, 256, None, True),
]


@pytest.mark.parametrize("NI,H,W,Cin,Cout,act,bias", SHAPES)
def test_winograd_accuracy_vs_fp64(NI, H, W, Cin, Cout, act, bias):
    from mdqe_cvpr2023_amd import ops
    x, w, b = _data(NI, H, W, Cin, Cout, H * W + Cin)
    if not bias:
        b = torch.zeros(Cout)
    ref = _ref64(x, w, b, act)
    wr, wd = _pair(w)
    xg, bg = x.cuda(), (b.cuda() if bias else None)
    yw = ops.conv2d_nhwc(xg, wr, bg, 1, 1, act=act).cpu().double()
    yd = ops.conv2d_nhwc(xg, wd, bg, 1, 1, act=act).cpu().double()
    s = float(ref.abs().max())
    e_w, e_d = float((yw - ref).abs().max()) / s, float((yd - ref).abs().max()) / s
    assert e_w < 2e-6, (e_w, e_d)
    assert e_w <= 4 * e_d, (e_w, e_d)
    assert not torch.equal(yw, yd)                      # the registered weight really took the other arithmetic


def test_winograd_image_strided_view():
    """Mask-head lay1 reads the 1/32 level as a view into the encoder tokens (images N x C floats apart, engine._mask_features)."""
    from mdqe_cvpr2023_amd import ops
    NI, H, W, C, N = 3, 15, 27, 256, 15 * 27 + 700
    g = torch.Generator().manual_seed(5)
    tok = torch.randn(NI, N, C, generator=g)
    w = torch.randn(C, 3, 3, C, generator=g) / (9 * C) ** 0.5
    b = torch.randn(C, generator=g)
    s0 = 500
    x = tok[:, s0:s0 + H * W].reshape(NI, H, W, C)
    ref = _ref64(x, w, b, None)
    wr, wd = _pair(w)
    tg = tok.cuda()
    xv = tg[:, s0:s0 + H * W].view(NI, H, W, C)
    assert xv.stride(0) == N * C
    yw = ops.conv2d_nhwc(xv, wr, b.cuda(), 1, 1).cpu().double()
    yd = ops.conv2d_nhwc(xv, wd, b.cuda(), 1, 1).cpu().double()
    s = float(ref.abs().max())
    e_w, e_d = float((yw - ref).abs().max()) / s, float((yd - ref).abs().max()) / s
    assert e_w < 2e-6 and e_w <= 4 * e_d, (e_w, e_d)
    # and the same bits as on a dense copy of the view
    assert torch.equal(ops.conv2d_nhwc(xv.contiguous(), wr, b.cuda(), 1, 1).cpu().double(), yw)


def test_winograd_frames_independent_and_deterministic():
    """Any subset of frames equals the matching rows of the full batch bit for bit, across image-group boundaries (45 x 80 x 256: four
    images per group, so 9 frames are three groups); two runs give equal bits."""
    from mdqe_cvpr2023_amd import _lib, ops
    NI, H, W, C = 9, 45, 80, 256
    assert _lib.lib.mdqe_winograd_workspace_bytes(NI, H, W, C, C) < _lib.lib.mdqe_winograd_workspace_bytes(1, H, W, C, C) * NI
    x, w, b = _data(NI, H, W, C, C, 77)
    wr, _ = _pair(w)
    xg, bg = x.cuda(), b.cuda()
    full = ops.conv2d_nhwc(xg, wr, bg, 1, 1, act="relu")
    again = ops.conv2d_nhwc(xg, wr, bg, 1, 1, act="relu")
    assert torch.equal(full, again)
    for lo, hi in ((0, 1), (3, 7), (2, 9), (8, 9), (0, 5)):
        part = ops.conv2d_nhwc(xg[lo:hi].contiguous(), wr, bg, 1, 1, act="relu")
        assert torch.equal(part, full[lo:hi]), (lo, hi)


def test_winograd_routing():
    """The split-precision modes, an unregistered weight, the MDQE_WINOGRAD switch, a residual, and a weight modified in place all take the
    direct kernel (equal bits to it); the registered weight in the exact fp32 mode does not."""
    from mdqe_cvpr2023_amd import ops
    x, w, b = _data(2, 23, 40, 256, 256, 3)
    wr, wd = _pair(w)
    xg, bg = x.cuda(), b.cuda()
    direct = ops.conv2d_nhwc(xg, wd, bg, 1, 1, act="relu")
    assert not torch.equal(ops.conv2d_nhwc(xg, wr, bg, 1, 1, act="relu"), direct)
    for mode in ("f16x3", "f16"):
        with ops.gemm_precision(mode):
            assert torch.equal(ops.conv2d_nhwc(xg, wr, bg, 1, 1, act="relu"), ops.conv2d_nhwc(xg, wd, bg, 1, 1, act="relu")), mode
    prev = ops.WINOGRAD
    ops.WINOGRAD = False
    try:
        assert torch.equal(ops.conv2d_nhwc(xg, wr, bg, 1, 1, act="relu"), direct)
    finally:
        ops.WINOGRAD = prev
    r = torch.randn(2, 23, 40, 256).cuda()
    assert torch.equal(ops.conv2d_nhwc(xg, wr, bg, 1, 1, residual=r), ops.conv2d_nhwc(xg, wd, bg, 1, 1, residual=r))
    wr.mul_(1.0)                                        # in-place update: the cached transform is dropped
    assert ops._wino_u(wr) is None
    assert torch.equal(ops.conv2d_nhwc(xg, wr, bg, 1, 1, act="relu"), direct)


@pytest.mark.parametrize("Cin,Cout", [(256, 512), (512, 256)])
def test_winograd_cin_ne_cout_across_groups(Cin, Cout):
    """Cin != Cout (V and M planes of different widths) over several image groups (45 x 80 with 768 channels in + out: two images per
    group, so 3 frames are two groups): accuracy against fp64 and against the direct kernel, and a subset across the group boundary equal
    to the matching rows of the full batch."""
    from mdqe_cvpr2023_amd import _lib, ops
    NI, H, W = 3, 45, 80
    assert _lib.lib.mdqe_winograd_workspace_bytes(NI, H, W, Cin, Cout) < _lib.lib.mdqe_winograd_workspace_bytes(1, H, W, Cin, Cout) * NI
    x, w, b = _data(NI, H, W, Cin, Cout, Cin + 3 * Cout)
    ref = _ref64(x, w, b, "relu")
    wr, wd = _pair(w)
    xg, bg = x.cuda(), b.cuda()
    yw = ops.conv2d_nhwc(xg, wr, bg, 1, 1, act="relu")
    yd = ops.conv2d_nhwc(xg, wd, bg, 1, 1, act="relu").cpu().double()
    s = float(ref.abs().max())
    e_w, e_d = float((yw.cpu().double() - ref).abs().max()) / s, float((yd - ref).abs().max()) / s
    assert e_w < 2e-6 and e_w <= 4 * e_d, (e_w, e_d)
    for lo, hi in ((1, 3), (2, 3)):
        assert torch.equal(ops.conv2d_nhwc(xg[lo:hi].contiguous(), wr, bg, 1, 1, act="relu"), yw[lo:hi]), (lo, hi)


def test_winograd_unaligned_out_takes_direct_kernel():
    """An `out` view whose rows start off a 16-byte boundary: the direct kernel (which takes unaligned operands) computes it, with its bits."""
    from mdqe_cvpr2023_amd import ops
    x, w, b = _data(2, 12, 20, 256, 256, 11)
    wr, wd = _pair(w)
    xg, bg = x.cuda(), b.cuda()
    buf = torch.zeros(2, 12, 20, 256 + 1).cuda()
    out = buf[..., 1:]                                   # rows 257 floats apart, first row at +4 bytes
    y = ops.conv2d_nhwc(xg, wr, bg, 1, 1, act="relu", out=out)
    direct = ops.conv2d_nhwc(xg, wd, bg, 1, 1, act="relu")
    assert torch.equal(y, direct)
