"""CPU: the Winograd F(2x2,3x3) arithmetic of csrc/winograd.hip, emulated in torch with the kernels' fp32 operation order (weight transform
in double, rounded once; input / output transforms in fp32; fp32 plane products), held to an fp64 convolution.  Its error must stay
within a small multiple of the direct fp32 convolution's on the same data -- the reason the product runs F(2x2) and not F(4x4)."""
import pytest
import torch
import torch.nn.functional as F


def wino_weight(w):
    """w [Cout, 3, 3, Cin] -> U [16, Cout, Cin] = G g G^T in double, rounded once (wino_weight_kernel)."""
    g = w.double()
    t = torch.stack([g[:, 0], 0.5 * (g[:, 0] + g[:, 1] + g[:, 2]), 0.5 * (g[:, 0] - g[:, 1] + g[:, 2]), g[:, 2]], 1)   # [Co, 4, 3, Ci]
    u = torch.stack([t[:, :, 0], 0.5 * (t[:, :, 0] + t[:, :, 1] + t[:, :, 2]), 0.5 * (t[:, :, 0] - t[:, :, 1] + t[:, :, 2]), t[:, :, 2]], 2)
    return u.float().permute(1, 2, 0, 3).reshape(16, w.shape[0], w.shape[3]).contiguous()


def wino_conv(x, w, b):
    """x [NI, H, W, Cin] fp32 NHWC, w [Cout, 3, 3, Cin] -> [NI, H, W, Cout] (stride 1, pad 1), the kernels' order of operations."""
    NI, H, W, C = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = torch.zeros(NI, 2 * th + 2, 2 * tw + 2, C)
    xp[:, 1:H + 1, 1:W + 1] = x
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                     # [NI, th, tw, C, 4 (row), 4 (col)]
    e = [d[..., 0, :] - d[..., 2, :], d[..., 1, :] + d[..., 2, :], d[..., 2, :] - d[..., 1, :], d[..., 1, :] - d[..., 3, :]]
    V = []
    for a in range(4):
        r = e[a]
        V += [r[..., 0] - r[..., 2], r[..., 1] + r[..., 2], r[..., 2] - r[..., 1], r[..., 1] - r[..., 3]]
    V = torch.stack(V, 0).reshape(16, -1, C)                   # [16, T, Cin]
    M = torch.bmm(V, wino_weight(w).transpose(1, 2))           # [16, T, Cout], fp32
    m = M.reshape(4, 4, NI, th, tw, -1)
    q = [(m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]]
    y = torch.empty(NI, th, 2, tw, 2, M.shape[-1])
    for a in range(2):
        y[:, :, a, :, 0] = ((q[a][0] + q[a][1]) + q[a][2]) + b
        y[:, :, a, :, 1] = ((q[a][1] - q[a][2]) - q[a][3]) + b
    return y.reshape(NI, 2 * th, 2 * tw, -1)[:, :H, :W]


@pytest.mark.parametrize("NI,H,W,Cin,Cout", [(3, 12, 20, 256, 256), (2, 24, 40, 256, 256), (1, 48, 80, 128, 128), (1, 15, 27, 256, 256),
                                             (2, 7, 9, 128, 512)])
def test_winograd_f2x2_error_vs_fp64(NI, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(H * W + Cin + Cout)
    x = torch.randn(NI, H, W, Cin, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g)
    x_nchw, w_oihw = x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2)
    ref = F.conv2d(x_nchw.double(), w_oihw.double(), b.double(), 1, 1).permute(0, 2, 3, 1)
    direct = F.conv2d(x_nchw, w_oihw, b, 1, 1).permute(0, 2, 3, 1)
    wino = wino_conv(x, w, b)
    s = float(ref.abs().max())
    e_dir = float((direct.double() - ref).abs().max()) / s
    e_win = float((wino.double() - ref).abs().max()) / s
    assert e_win < 2e-6, (e_win, e_dir)
    assert e_win <= 4 * e_dir + 1e-7, (e_win, e_dir)


def test_winograd_weight_transform_exact_on_grid():
    """U = G g G^T on weights that are multiples of 1/4: every intermediate is exact, so U must equal the fp64 product bit for bit."""
    g = torch.Generator().manual_seed(0)
    w = torch.randint(-64, 64, (8, 3, 3, 4), generator=g).float() / 4
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
    ref = torch.einsum("ar,nrsc,bs->abnc", G, w.double(), G).reshape(16, 8, 4)
    assert torch.equal(wino_weight(w).double(), ref)


def test_winograd_workspace_query():
    """The workspace query covers V and M of one image group plus the zero bias; the group never grows with NI past its cap."""
    from mdqe_cvpr2023_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    h = _lib.load_library()
    one = h.mdqe_winograd_workspace_bytes(1, 45, 80, 256, 256)
    assert one >= 16 * 23 * 40 * 512 * 4 + 256 * 4
    assert h.mdqe_winograd_workspace_bytes(40, 45, 80, 256, 256) <= (128 << 20) + 4096      # grouped: stays within the cache budget
    assert h.mdqe_winograd_workspace_bytes(4, 45, 80, 256, 256) == h.mdqe_winograd_workspace_bytes(40, 45, 80, 256, 256)
    assert h.mdqe_winograd_workspace_bytes(0, 45, 80, 256, 256) == 0
