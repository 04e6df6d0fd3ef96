"""The band-mapped dense final masks (final_mask_band_kernel, what mdqe_final_masks_u8 launches) against the flat kernel it replaces
(final_mask_kernel, MDQE_FINAL_MASK_FLAT=1): the same bytes, compared with torch.equal over the WHOLE output buffer, so rows and frames
outside the window must keep what they held.

Both kernels take the pixel from csrc/final_mask.h; what differs is who computes which pixel and how the bytes leave -- a thread of the
band kernel owns 4 consecutive pixels of a row for all tracks and stores a track's four bytes as one dword where the address allows.
Hence the cases: odd widths (rows that start at every alignment; a last group of 1 to 3 pixels), an output base at +1 byte, an output
height the band does not divide (37 = 19 + 18 rows, 96 = 13 x 7 + 5), a down-scale, a window written at a frame offset into a longer
plane, 0 / 1 / 3 / 17 selected rows with a permuted index that repeats a row, and logits at the threshold (exact zeros and +-1e-7,
where the sigmoid is 0.5 or one rounding away from it).

Wall time on one MI355X: well under a second per case (12 x 20 logits, at most 96 x 160 outputs).
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HM, WM, FACTOR, N_TRACKS = 12, 20, 4, 9
CROPS = [(45, 77), (48, 80)]
OUTPUTS = [(37, 53), (48, 80), (96, 160), (23, 40)]
CANARY = 7


def _logits(Fw, seed):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(N_TRACKS, Fw, HM, WM, generator=g) * 3.0
    near = torch.tensor([0.0, 1e-7, -1e-7, 0.0])
    pick = torch.randint(0, 16, lg.shape, generator=g)
    lg = torch.where(pick < 4, near[pick.clamp(max=3)], lg)          # a quarter of the logits sit at the threshold
    lg[1] = 0.0                                                      # whole maps: sigmoid == 0.5 exactly -> no bit
    lg[2] = 1e-7                                                     # one rounding from the threshold, on either side
    lg[3] = -1e-7
    return lg.cuda()


def _rows(n_sel):
    """Selected rows: a permutation of the tracks that repeats a row (n_sel >= 3)."""
    base = [5, 2, 5, 8, 0, 1, 3, 7, 4, 6, 2, 2, 8, 1, 0, 3, 5]
    rows = [4] if n_sel == 1 else base[:n_sel]
    return torch.tensor(rows, dtype=torch.int32, device="cuda")


def _run(ops, monkeypatch, flat, lg, rows, h, w, Ho, Wo, f_off, L, byte_off):
    """One call into a canary-filled [max(n_sel, 1) + 1, L, Ho, Wo] plane that starts `byte_off` bytes into its allocation."""
    if flat:
        monkeypatch.setenv("MDQE_FINAL_MASK_FLAT", "1")
    else:
        monkeypatch.delenv("MDQE_FINAL_MASK_FLAT", raising=False)
    n_rows = max(int(rows.numel()), 1) + 1
    buf = torch.full((n_rows * L * Ho * Wo + byte_off,), CANARY, dtype=torch.uint8, device="cuda")
    out = buf[byte_off:].view(n_rows, L, Ho, Wo)
    ops.final_masks(lg, rows, FACTOR, h, w, Ho, Wo, out, f_off)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Fw", [1, 2])
@pytest.mark.parametrize("Ho,Wo", OUTPUTS)
def test_band_kernel_writes_the_flat_kernels_bytes(monkeypatch, Ho, Wo, Fw):
    from mdqe_cvpr2023_amd import ops
    lg = _logits(Fw, seed=100 * Ho + Fw)
    f_off, L = 2, Fw + 4                                             # the window sits inside a longer plane
    some_set = False
    for h, w in CROPS:
        for n_sel in (0, 1, 3, 17):
            rows = _rows(n_sel)
            for byte_off in (0, 1):
                want = _run(ops, monkeypatch, True, lg, rows, h, w, Ho, Wo, f_off, L, byte_off)
                got = _run(ops, monkeypatch, False, lg, rows, h, w, Ho, Wo, f_off, L, byte_off)
                what = f"crop {(h, w)} out {(Ho, Wo)} n_sel {n_sel} Fw {Fw} base +{byte_off}"
                assert torch.equal(got, want), what
                # the window's frames of the selected rows are masks; everything else still holds the canary
                win = got[:n_sel, f_off:f_off + Fw]
                assert bool((win <= 1).all()), what
                assert bool((got[:n_sel, :f_off] == CANARY).all()) and bool((got[:n_sel, f_off + Fw:] == CANARY).all()), what
                assert bool((got[n_sel:] == CANARY).all()), what
                some_set = some_set or bool(win.any())
                if n_sel >= 3:
                    assert torch.equal(win[0], win[2]), what         # rows 0 and 2 select the same track
    assert some_set                                                  # (the comparison is not between two empty planes)


def test_threshold_maps_have_no_bit_and_repeat_runs_agree(monkeypatch):
    """Maps that are 0 or -1e-7 everywhere: sigmoid(v) > 0.5 is false on both (0.5 exactly, and at most 0.5), so neither has a bit.  The
    map at +1e-7 is the threshold's other side -- whether fp32 rounds its sigmoid to 0.5 or just above is final_mask_bit's business, and
    the only claim here is that both kernels decide it alike.  And two runs of the band kernel give the same bytes."""
    from mdqe_cvpr2023_amd import ops
    lg = _logits(2, seed=5)
    rows = torch.tensor([1, 3, 2, 0], dtype=torch.int32, device="cuda")
    a = _run(ops, monkeypatch, False, lg, rows, 45, 77, 37, 53, 1, 4, 1)
    b = _run(ops, monkeypatch, False, lg, rows, 45, 77, 37, 53, 1, 4, 1)
    assert torch.equal(a, b)
    assert not bool(a[:2, 1:3].any())
    assert bool(a[3, 1:3].any())
    assert torch.equal(a, _run(ops, monkeypatch, True, lg, rows, 45, 77, 37, 53, 1, 4, 1))
