"""CPU: the Winograd F(2x2,3x3) arithmetic of csrc/winograd.hip, emulated in torch with the kernels' fp32 operation order (weight transform
in double, rounded once; input / output transforms in fp32; fp32 plane products), held to an fp64 convolution.  Its error must stay
within a small multiple of the direct fp32 convolution's on the same data -- the reason the product runs F(2x2) and not F(4x4)."""
import pytest
import torch
import torch.nn.functional as F

# the emulation lives beside the float64 references and bounds that tests/test_conv_spatial_*.py hold the kernels to
from _conv_spatial_ref import wino_eval as wino_conv, wino_weight


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
