"""What track outlines cost: one tracker window's label stage (ops.final_label_map) alone, and with the polygon launches and their
read-back behind it (merge.polygon_rings: ops.label_polygons with the default caps, the sync on the totals, the rings to pinned
host memory).  The workload of tools/trails_ab.py: one window of 15 tracks x 30 frames of 360 x 640, the label generator of
tools/overlay_ab.py.  Beside it the host route a caller has today: the label map read back into pinned memory, then
polygons.polygons_from_labels on the host, whose output must equal the kernel's.  Tables are appended to OUT when given."""
import os, sys, statistics, time
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import merge, ops
from mdqe_cvpr2023_amd.polygons import Polygons, polygons_from_labels


def emit(lines):
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as fh:
            fh.write("\n".join(lines) + "\n\n")
    print("\n".join(lines))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps     # us per call


def walled(fn, reps):
    """us per call on the host's clock, for the variants that end in a host sync of their own."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def launches():
    h, w, Fw, n = 360, 640, 30, 15
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/overlay_ab.py)
    g = torch.Generator().manual_seed(0)
    lg = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    spec = Polygons()
    pin = torch.empty(lab.shape, dtype=torch.uint8, pin_memory=True)
    kept = {}

    def label_stage():
        ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)

    def with_kernels():                                                      # the launches alone, default caps: nothing read back, no sync
        label_stage()
        kept["dev"] = ops.label_polygons(lab, n, 0)

    label_stage()
    V, R = (int(v) for v in ops.label_polygons(lab, n, 0)[2].tolist())

    def with_kernels_fit():                                                  # ... with caps that hold the window's totals
        label_stage()
        ops.label_polygons(lab, n, 0, max(V, 1), max(R, 1))

    def with_polygons():                                                     # what a window pays: launches, two syncs, the rings on the host
        label_stage()
        kept["tp"] = merge.polygon_rings(lab, 0, n, Fw, (h, w), spec, None, 0)

    def read_back():
        label_stage()
        pin.copy_(lab, non_blocking=True)
        torch.cuda.current_stream().synchronize()

    def label_synced():
        label_stage()
        torch.cuda.current_stream().synchronize()
    dev_variants = [("label stage alone", label_stage), ("+ polygon launches, default caps (no read-back)", with_kernels),
                    ("+ polygon launches, caps = the totals (no read-back)", with_kernels_fit)]
    host_variants = [("label stage alone, synced", label_synced), ("+ polygons (launches, sync, rings on the host)", with_polygons),
                     ("+ read-back of the map (host route, first half)", read_back)]
    reps = {}
    for name, fn in dev_variants + host_variants:
        for _ in range(5): fn()
        torch.cuda.synchronize()
        reps[name] = max(10, int(0.25e6 / max(walled(fn, 10), 1.0)) + 1)
    res = {name: [] for name, _ in dev_variants + host_variants}
    for r in range(7):
        for name, fn in (dev_variants if r % 2 == 0 else dev_variants[::-1]):       # alternating order
            res[name].append(timed(fn, reps[name]))
        for name, fn in (host_variants if r % 2 == 0 else host_variants[::-1]):
            res[name].append(walled(fn, reps[name]))
    med = {k: statistics.median(x) for k, x in res.items()}
    # the host route's second half, on what was read back; its output must be the kernel's
    with_polygons()
    read_back()
    host_t = []
    for _ in range(3):
        t0 = time.perf_counter()
        hp = polygons_from_labels(pin.numpy(), n)
        host_t.append((time.perf_counter() - t0) * 1e6)
    tp = kept["tp"]
    same = hp == tp
    assert (V, R) == tuple(int(v) for v in kept["dev"][2].tolist())
    cap_v, cap_r = int(kept["dev"][0].shape[0]), int(kept["dev"][1].shape[0])
    rounds = max(cap_v - 1, 0).bit_length()
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d; totals V = %d vertices, R = %d rings (%d holes), %d bytes on the host;"
             % (n, Fw, h, w, V, R, int(tp.rings[:, 4].sum()), tp.xy.nbytes + tp.rings.nbytes),
             "# default caps %d vertices / %d rings (no retry: %s), %d ranking rounds; the label map itself is %d bytes"
             % (cap_v, cap_r, V <= cap_v and R <= cap_r, rounds, Fw * h * w),
             "# the synthetic generator's regions are redrawn per frame and are blob-like, 15 of them competing for every pixel: %d rings and %d corners per"
             % (R // Fw, V // Fw),
             "# frame, every slanted edge a staircase of corners; where the default caps overflow, the first call only counts (its link pass walks rings) and",
             "# merge.polygon_rings calls again with the totals as caps",
             "# us per call; 7 passes over all variants in one process, order alternating; medians",
             "# device rows: device events around >= 0.25 s of back-to-back calls; host rows: the host's clock around calls that each end in a sync",
             "%-58s %6s %9s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "- alone", "/ alone")]
    for group, base in ((dev_variants, med[dev_variants[0][0]]), (host_variants, med[host_variants[0][0]])):
        for name, _ in group:
            x = res[name]
            lines.append("%-58s %6d %9.1f %9.1f %9.1f %9.1f %8.2f" % (name, reps[name], med[name], min(x), max(x), med[name] - base, med[name] / base))
    b_dev, b_host = med[dev_variants[0][0]], med[host_variants[0][0]]
    lines.append("host route: the read-back above (%.1f us beyond the synced stage) + polygons.polygons_from_labels on the host: %.0f us (min of 3); "
                 "output equal to the kernel's: %s" % (med[host_variants[2][0]] - b_host, min(host_t), same))
    lines.append("so the polygon launches with caps that fit cost %.2fx the label stage on the device (%.1f us beside %.1f); a window with polygons "
                 "on the host costs %.2fx the synced label stage; the host route costs %.1fx"
                 % ((med[dev_variants[2][0]] - b_dev) / b_dev, med[dev_variants[2][0]] - b_dev, b_dev, med[host_variants[1][0]] / b_host,
                    (med[host_variants[2][0]] + min(host_t)) / b_host))
    emit(lines)
    if not same:
        raise SystemExit("the host route's polygons differ from the kernel's")


if __name__ == "__main__":
    launches()
