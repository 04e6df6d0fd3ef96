"""A/B of the final-mask kernels with and without geometry on one tracker window of 15 tracks: the shipped 360p one (30 frames of
360 x 640) or, `final_mask_geom_ab.py OUT H W FRAMES`, one of FRAMES frames of H x W (output size = frame size).  MDQE_HIP_LIB selects the
library build, so two builds are compared by running the tool once per build."""
import os, sys, statistics
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops

h, w, Fw = (int(v) for v in sys.argv[2:5]) if len(sys.argv) > 4 else (360, 640, 30)
n, Hm, Wm, Ho, Wo = 15, (h + 31) // 32 * 8, (w + 31) // 32 * 8, h, w          # (the stride-4 map of the frame padded to a multiple of 32)
g = torch.Generator().manual_seed(0)
lg = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
idx = torch.arange(n, dtype=torch.int32, device="cuda")
out = torch.empty(n, Fw, Ho, Wo, dtype=torch.uint8, device="cuda")
geom = torch.empty(n * Fw, 5, dtype=torch.int32, device="cuda")
cap = 4 * (Ho + Wo) + 64
ar_x, ar_y = torch.arange(Wo, device="cuda"), torch.arange(Ho, device="cuda")

def u8(): ops.final_masks(lg, idx, 4, h, w, Ho, Wo, out, 0)
def u8_geom(): ops.final_masks_geom(lg, idx, 4, h, w, Ho, Wo, out, 0, geom=geom)
def rle(): ops.final_masks_rle(lg, idx, 4, h, w, Ho, Wo, cap)
def rle_geom(): ops.final_masks_rle_geom(lg, idx, 4, h, w, Ho, Wo, cap, geom=geom)
def u8_then_torch():
    ops.final_masks(lg, idx, 4, h, w, Ho, Wo, out, 0)
    pm = out.view(torch.bool).view(n * Fw, Ho, Wo)
    area = pm.flatten(1).sum(1)
    xa, ya = pm.any(1), pm.any(2)
    has = xa.any(1)
    x0 = torch.where(xa, ar_x, Wo).min(1)[0]; x1 = torch.where(xa, ar_x, -1).max(1)[0] + 1
    y0 = torch.where(ya, ar_y, Ho).min(1)[0]; y1 = torch.where(ya, ar_y, -1).max(1)[0] + 1
    return area, torch.stack([x0, y0, x1, y1], 1).float() * has[:, None]

variants = [("mdqe_final_masks_u8", u8), ("mdqe_final_masks_u8_geom", u8_geom), ("mdqe_final_masks_rle", rle),
            ("mdqe_final_masks_rle_geom", rle_geom), ("mdqe_final_masks_u8 + torch sum/any/min/max", u8_then_torch)]

def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps     # us per call

# sanity: same bits, and the torch alternative computes the same geometry
u8(); ref = out.clone(); u8_geom(); assert torch.equal(out, ref)
area, boxes = u8_then_torch()
from mdqe_cvpr2023_amd import rle as R
bx, ar = R.geom_to_boxes(geom)
assert torch.equal(ar, area.cpu()) and torch.equal(bx, boxes.cpu())
reps = {}
for name, fn in variants:
    for _ in range(5): fn()
    torch.cuda.synchronize()
    t = timed(fn, 20)
    reps[name] = max(20, int(0.25e6 / t) + 1)
res = {name: [] for name, _ in variants}
for r in range(7):
    for name, fn in variants:
        res[name].append(timed(fn, reps[name]))
lines = ["# one tracker window: n = %d tracks x %d frames, Hm x Wm = %d x %d, h, w = Ho, Wo = %d, %d (%d masks, %.1f MB of uint8)"
         % (n, Fw, Hm, Wm, Ho, Wo, n * Fw, n * Fw * Ho * Wo / 1e6),
         "# us per call, device events around >= 0.25 s of back-to-back launches, 7 alternations of all variants in one process",
         "# set pixels: %.1f %% of all; empty masks: %d of %d" % (100.0 * float(ar.sum()) / (n * Fw * Ho * Wo), int((ar == 0).sum()), n * Fw),
         "%-46s %6s %9s %9s %9s" % ("variant", "reps", "median", "min", "max")]
med = {}
for name, _ in variants:
    v = res[name]; med[name] = statistics.median(v)
    lines.append("%-46s %6d %9.1f %9.1f %9.1f" % (name, reps[name], med[name], min(v), max(v)))
lines.append("u8_geom / u8                = %.3f" % (med["mdqe_final_masks_u8_geom"] / med["mdqe_final_masks_u8"]))
lines.append("rle_geom / rle              = %.3f" % (med["mdqe_final_masks_rle_geom"] / med["mdqe_final_masks_rle"]))
lines.append("u8_geom / (u8 + torch)      = %.3f   (gate: < 1)" % (med["mdqe_final_masks_u8_geom"] / med["mdqe_final_masks_u8 + torch sum/any/min/max"]))
if len(sys.argv) > 1:                          # final_mask_geom_ab.py [OUT]: the table also goes to the file OUT
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines))
assert med["mdqe_final_masks_u8_geom"] < med["mdqe_final_masks_u8 + torch sum/any/min/max"]
