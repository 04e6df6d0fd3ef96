"""A/B of the two forms a tracker window's final masks leave the device in: one uint8 plane per track (mdqe_final_masks_u8 /
mdqe_final_masks_u8_geom, the yardstick) against one label plane per frame (mdqe_final_label_map_u8), with and without geometry, the
label kernel in its shipped cache-read and its LDS-staged form (MDQE_LABEL_MAP_STAGE=1), and the device-to-host copy of each form's output into
pinned memory.  One window of 15 tracks: the shipped 360p one (30 frames of 360 x 640) or, `label_map_ab.py OUT H W FRAMES`, one of
FRAMES frames of H x W (output size = frame size).  The table is appended to OUT when given (one file for several windows)."""
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
lab = torch.empty(Fw, Ho, Wo, dtype=torch.uint8, device="cuda")
geom = torch.empty(n * Fw, 5, dtype=torch.int32, device="cuda")
h_out = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)
h_lab = torch.empty(lab.shape, dtype=torch.uint8, pin_memory=True)


def stage(on):
    if on:
        os.environ["MDQE_LABEL_MAP_STAGE"] = "1"      # (read by the entry point at every call; unset = the shipped cache-read form)
    else:
        os.environ.pop("MDQE_LABEL_MAP_STAGE", None)

def u8(): ops.final_masks(lg, idx, 4, h, w, Ho, Wo, out, 0)
def u8_geom(): ops.final_masks_geom(lg, idx, 4, h, w, Ho, Wo, out, 0, geom=geom)
def label_staged(): stage(True); ops.final_label_map(lg, idx, 4, h, w, Ho, Wo, lab, 0)
def label_staged_geom(): stage(True); ops.final_label_map(lg, idx, 4, h, w, Ho, Wo, lab, 0, geom=geom)
def label_cached(): stage(False); ops.final_label_map(lg, idx, 4, h, w, Ho, Wo, lab, 0)
def label_cached_geom(): stage(False); ops.final_label_map(lg, idx, 4, h, w, Ho, Wo, lab, 0, geom=geom)
def d2h_dense(): h_out.copy_(out, non_blocking=True)
def d2h_label(): h_lab.copy_(lab, non_blocking=True)

variants = [("mdqe_final_masks_u8", u8), ("mdqe_final_masks_u8_geom", u8_geom),
            ("mdqe_final_label_map_u8 staged", label_staged), ("mdqe_final_label_map_u8 staged + geom", label_staged_geom),
            ("mdqe_final_label_map_u8 cache-read", label_cached), ("mdqe_final_label_map_u8 cache-read + geom", label_cached_geom),
            ("D2H dense planes -> pinned", d2h_dense), ("D2H label map -> pinned", d2h_label)]

def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps     # us per call

# sanity: the map is the union of the dense masks, names a track whose mask holds the pixel, both forms agree, geometry = pixel counts
u8()
masks = out.view(torch.bool)
label_staged_geom(); ref, g_staged = lab.clone(), geom.clone()
label_cached_geom()
torch.cuda.synchronize()
assert torch.equal(lab, ref) and torch.equal(geom, g_staged)
assert torch.equal(ref != 0, masks.any(0))
assert bool(masks.gather(0, (ref.long() - 1).clamp(min=0)[None])[0][ref != 0].all())
areas = torch.stack([(ref == t + 1).flatten(1).sum(1) for t in range(n)])
assert torch.equal(g_staged.view(n, Fw, 5)[..., 0].long(), areas)
claimed = masks.sum(0)
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
stage(False)
dense_b, label_b = n * Fw * Ho * Wo, Fw * Ho * Wo
bytes_out = {"mdqe_final_masks_u8": dense_b, "mdqe_final_masks_u8_geom": dense_b, "D2H dense planes -> pinned": dense_b}
lines = ["# one tracker window: n = %d tracks x %d frames, Hm x Wm = %d x %d, h, w = Ho, Wo = %d, %d; logits read %.1f MB"
         % (n, Fw, Hm, Wm, Ho, Wo, lg.numel() * 4 / 1e6),
         "# written / copied: dense %.1f MB (%d planes), label map %.1f MB (%d planes)" % (dense_b / 1e6, n * Fw, label_b / 1e6, Fw),
         "# us per call, device events around >= 0.25 s of back-to-back calls, 7 alternations of all variants in one process",
         "# pixels no track claims: %.1f %%, claimed by two or more: %.1f %%; labels with an empty region: %d of %d"
         % (100.0 * float((claimed == 0).float().mean()), 100.0 * float((claimed >= 2).float().mean()), int((areas == 0).sum()), n * Fw),
         "%-44s %6s %9s %9s %9s %12s" % ("variant", "reps", "median", "min", "max", "GB/s out")]
med = {}
for name, _ in variants:
    v = res[name]; med[name] = statistics.median(v)
    lines.append("%-44s %6d %9.1f %9.1f %9.1f %12.1f" % (name, reps[name], med[name], min(v), max(v), bytes_out.get(name, label_b) / med[name] / 1e3))
best = min(med["mdqe_final_label_map_u8 staged + geom"], med["mdqe_final_label_map_u8 cache-read + geom"])
lines.append("label staged + geom / u8_geom      = %.3f   (expected <= 1)" % (med["mdqe_final_label_map_u8 staged + geom"] / med["mdqe_final_masks_u8_geom"]))
lines.append("label cache-read + geom / u8_geom  = %.3f" % (med["mdqe_final_label_map_u8 cache-read + geom"] / med["mdqe_final_masks_u8_geom"]))
lines.append("label staged / u8                  = %.3f" % (med["mdqe_final_label_map_u8 staged"] / med["mdqe_final_masks_u8"]))
lines.append("label cache-read / staged          = %.3f   (geom: %.3f)" % (med["mdqe_final_label_map_u8 cache-read"] / med["mdqe_final_label_map_u8 staged"],
             med["mdqe_final_label_map_u8 cache-read + geom"] / med["mdqe_final_label_map_u8 staged + geom"]))
lines.append("kernel + copy per window: dense %.1f us, label map %.1f us" % (med["mdqe_final_masks_u8_geom"] + med["D2H dense planes -> pinned"],
             best + med["D2H label map -> pinned"]))
if len(sys.argv) > 1:                          # label_map_ab.py [OUT]: the table is also appended to the file OUT
    with open(sys.argv[1], "a") as fh:
        fh.write("\n".join(lines) + "\n\n")
print("\n".join(lines))
