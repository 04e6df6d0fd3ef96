"""A/B of the two kernels on the path from mask features to final masks, each against what it replaces, in one process on one device:

  * the mask head's up-sampling depthwise conv + 256 -> 32 projection as one kernel (ops.dwconv5x5_up2_pw) against the two launches
    (MDQE_MASK_HEAD_FUSED=0), on a 40-frame 360p pass and a 24-frame 640 x 1138 pass;
  * the band-mapped dense final masks (mdqe_final_masks_u8) against the flat kernel (MDQE_FINAL_MASK_FLAT=1) and against
    mdqe_final_masks_u8_geom, on the 15-track x 30-frame window of tools/final_mask_geom_ab.py at 360p and at 640 x 1138.

Device events around >= 0.2 s of back-to-back launches, 7 alternations of all variants of a group; medians and spread.
`mask_path_ab.py [OUT]`: the table also goes to the file OUT."""
import os, sys, statistics
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops

def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps     # us per call

def ab(title, variants, lines):
    """variants: [(name, fn)] -> {name: median us}; appends the group's table to lines."""
    reps = {}
    for name, fn in variants:
        for _ in range(5): fn()
        torch.cuda.synchronize()
        reps[name] = max(10, int(0.2e6 / timed(fn, 10)) + 1)
    res = {name: [] for name, _ in variants}
    for r in range(7):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            res[name].append(timed(fn, reps[name]))
    lines.append("## " + title)
    lines.append("%-58s %6s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "spread"))
    med = {}
    for name, _ in variants:
        v = res[name]; med[name] = statistics.median(v)
        lines.append("%-58s %6d %9.1f %9.1f %9.1f %7.2f%%" % (name, reps[name], med[name], min(v), max(v), 100.0 * (max(v) - min(v)) / med[name]))
    return med

def mask_head(NI, Hs, Ws, what, lines):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(NI, Hs, Ws, 256).cuda()
    wt, bias, tw, tb = (r(25, 256) * 0.2).cuda(), r(256).cuda(), (1.0 + 0.3 * r(256)).cuda(), r(256).cuda()
    pw, pb = (r(32, 256) / 16).cuda(), r(32).cuda()
    out = torch.empty(NI * 4 * Hs * Ws, 32, device="cuda")
    def fused():
        ops.MASK_HEAD_FUSED = True
        ops.dwconv5x5_up2_pw(x, wt, bias, tw, tb, pw, pb, out=out)
    def pair():
        ops.MASK_HEAD_FUSED = False
        ops.dwconv5x5_up2_pw(x, wt, bias, tw, tb, pw, pb, out=out)
    def dw_only(): ops.dwconv5x5(x, wt, bias, up2=True, tw=tw, tb=tb)
    pair(); want = out.clone(); out.zero_(); fused(); assert torch.equal(out, want), "fused mask head: bits differ"
    med = ab("mask head tail, %s: x [%d, %d, %d, 256] -> [%d, 32] (the tensor not stored: %.0f MB)"
             % (what, NI, Hs, Ws, out.shape[0], out.shape[0] * 1024 / 1e6),
             [("one kernel (mdqe_dwconv5x5_up2_pw_c256_f32)", fused), ("two launches (dw5_up2_c256_kernel + gemm N=32 K=256)", pair),
              ("  of which dw5_up2_c256_kernel alone", dw_only)], lines)
    ops.MASK_HEAD_FUSED = True
    a, b = med["one kernel (mdqe_dwconv5x5_up2_pw_c256_f32)"], med["two launches (dw5_up2_c256_kernel + gemm N=32 K=256)"]
    lines.append("one kernel / two launches = %.3f  (%.1f us saved per pass)" % (a / b, b - a))
    lines.append("")

def final_masks(h, w, Fw, what, lines):
    n, Hm, Wm, Ho, Wo = 15, (h + 31) // 32 * 8, (w + 31) // 32 * 8, h, w
    g = torch.Generator().manual_seed(0)
    lg = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    out = torch.empty(n, Fw, Ho, Wo, dtype=torch.uint8, device="cuda")
    geom = torch.empty(n * Fw, 5, dtype=torch.int32, device="cuda")
    def band():
        os.environ.pop("MDQE_FINAL_MASK_FLAT", None)
        ops.final_masks(lg, idx, 4, h, w, Ho, Wo, out, 0)
    def flat():
        os.environ["MDQE_FINAL_MASK_FLAT"] = "1"
        ops.final_masks(lg, idx, 4, h, w, Ho, Wo, out, 0)
    def u8_geom(): ops.final_masks_geom(lg, idx, 4, h, w, Ho, Wo, out, 0, geom=geom)
    flat(); want = out.clone(); out.zero_(); band(); assert torch.equal(out, want), "band-mapped final masks: bits differ"
    med = ab("final masks, %s: %d tracks x %d frames of %d x %d (%.1f MB of uint8; set pixels %.1f %%)"
             % (what, n, Fw, Ho, Wo, out.numel() / 1e6, 100.0 * float(want.float().mean())),
             [("mdqe_final_masks_u8 (final_mask_band_kernel)", band), ("MDQE_FINAL_MASK_FLAT=1 (final_mask_kernel)", flat),
              ("mdqe_final_masks_u8_geom", u8_geom)], lines)
    os.environ.pop("MDQE_FINAL_MASK_FLAT", None)
    a = med["mdqe_final_masks_u8 (final_mask_band_kernel)"]
    lines.append("band / flat = %.3f   band / u8_geom = %.3f" % (a / med["MDQE_FINAL_MASK_FLAT=1 (final_mask_kernel)"], a / med["mdqe_final_masks_u8_geom"]))
    lines.append("")

lines = ["# us per call; device events around >= 0.2 s of back-to-back launches; 7 alternations (order reversed every other round) of a",
         "# group's variants in one process; spread = (max - min) / median of the 7.  Equal bits are asserted before timing.", ""]
mask_head(40, 48, 80, "40-frame 360p pass", lines)
mask_head(24, 80, 144, "24-frame 640 x 1138 pass", lines)
final_masks(360, 640, 30, "360p window", lines)
final_masks(640, 1138, 30, "640 x 1138 window", lines)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
print("\n".join(lines))
