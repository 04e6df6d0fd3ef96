"""What track centroids and trails cost: one tracker window's label + overlay stage (ops.final_label_map, then ops.render_overlay; the
stage as it was, Style(trail=0)) alone, with the centroids behind the label map (ops.label_centroids into a point table), and with
the trail pass behind the painter (ops.render_trails: trail 16 and 64, width 1, 2 and 5; NV12 surfaces: ops.render_overlay_yuv and
ops.render_trails_yuv).  The workload of tools/crops_ab.py: one window of 15 tracks x 30 frames of 360 x 640 of the bench's synthetic
video, the label generator of tools/overlay_ab.py.  The point table's history columns hold the window's own centroids, repeated, so a
trail of 64 has 64 present points per track.  Beside it the host alternative a caller has today: the label map read back into pinned
memory, then the sums in numpy (held to the kernel's integers here).  Tables are appended to OUT when given."""
import os, sys, statistics, time
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops, render
from mdqe_cvpr2023_amd.preprocess import YuvFrames


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


def host_centroids(labels, n):
    """The rule of include/mdqe_hip.h on the host: per frame three bincounts."""
    Fw, Ho, Wo = labels.shape
    xs = np.broadcast_to(np.arange(Wo, dtype=np.int64), (Ho, Wo)).ravel()
    ys = np.broadcast_to(np.arange(Ho, dtype=np.int64)[:, None], (Ho, Wo)).ravel()
    mom = np.zeros((n, Fw, 3), dtype=np.int64)
    for f in range(Fw):
        l = labels[f].ravel()
        for c, w in enumerate((None, xs, ys)):
            mom[:, f, c] = np.bincount(l, weights=w, minlength=256)[1:n + 1].astype(np.int64)   # (sums below 2^53: exact in float64)
    m = mom[..., 0]
    pts = np.where(m[..., None] >= 1, (mom[..., 1:] + (m // 2)[..., None]) // np.maximum(m, 1)[..., None], -1).astype(np.int32)
    return mom, pts


def launches():
    from bench import synth_video
    h, w, Fw, n, TMAX = 360, 640, 30, 15, 64
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/overlay_ab.py)
    g = torch.Generator().manual_seed(0)
    lg = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    v = synth_video(0, Fw, seed=1).round().clamp(0, 255).to(torch.uint8)
    fr8 = v.cuda()
    pic = torch.empty(Fw, h, w, 3, dtype=torch.uint8, device="cuda")
    s = YuvFrames.empty(Fw, h, w, device="cuda")                             # luma from the green plane, chroma from sub-sampled red and blue
    s.y.copy_(v[:, 1])
    s.uv.copy_(torch.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(Fw, h // 2, w))
    spic = YuvFrames.empty(Fw, h, w, device="cuda")
    st = render.Style()
    pal, pal_y = st.palette_on("cuda"), st.palette_yuv_on("cuda", *s.meta()[2:])
    mom = torch.empty(n, Fw, 3, dtype=torch.int64, device="cuda")
    pts = torch.full((255, TMAX + Fw, 2), -1, dtype=torch.int32, device="cuda")
    # the history: the window's own centroids, repeated backwards
    ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
    ops.label_centroids(lab, n, 0, mom, pts, TMAX)
    for c in range(TMAX):
        pts[:n, TMAX - 1 - c] = pts[:n, TMAX + (Fw - 1 - c) % Fw]
    torch.cuda.synchronize()

    def stage(centroids=False, trail=0, width=2, surface=False):
        def run():
            ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
            if centroids:
                ops.label_centroids(lab, n, 0, mom, pts, TMAX)
            if surface:
                ops.render_overlay_yuv(lab, s, pal_y, spic, 0, st.a256, st.contour)
                if trail:
                    ops.render_trails_yuv(spic, pts, n, pal_y, Fw, 0, TMAX, trail, width)
            else:
                ops.render_overlay(lab, fr8, pal, pic, 0, st.a256, st.contour)
                if trail:
                    ops.render_trails(pic, pts, n, pal, Fw, 0, TMAX, trail, width)
        return run
    variants = [("label + overlay stage alone (trail = 0)", stage()),
                ("+ centroids", stage(True)),
                ("+ centroids + trails, trail 16, width 2", stage(True, 16, 2)),
                ("+ centroids + trails, trail 64, width 2", stage(True, 64, 2)),
                ("+ centroids + trails, trail 16, width 1", stage(True, 16, 1)),
                ("+ centroids + trails, trail 16, width 5", stage(True, 16, 5)),
                ("+ centroids + trails, trail 64, width 5", stage(True, 64, 5)),
                ("NV12: label + overlay stage alone", stage(surface=True)),
                ("NV12: + centroids + trails, trail 16, width 2", stage(True, 16, 2, True)),
                ("NV12: + centroids + trails, trail 64, width 5", stage(True, 64, 5, True))]
    pin = torch.empty(lab.shape, dtype=torch.uint8, pin_memory=True)

    def read_back():
        stage()()
        pin.copy_(lab, non_blocking=True)
    variants.append(("label + overlay stage + read-back of the map", read_back))
    reps = {}
    for name, fn in variants:
        for _ in range(5): fn()
        torch.cuda.synchronize()
        reps[name] = max(10, int(0.25e6 / timed(fn, 10)) + 1)
    res = {name: [] for name, _ in variants}
    for r in range(7):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):               # alternating order
            res[name].append(timed(fn, reps[name]))
    med = {k: statistics.median(x) for k, x in res.items()}
    base, base_y = med[variants[0][0]], med[variants[7][0]]
    # the host's numpy pass on what was read back, held to the kernel's integers
    stage(True)()
    read_back()
    torch.cuda.synchronize()
    host_t = []
    for _ in range(3):
        t0 = time.perf_counter()
        hm, hp = host_centroids(pin.numpy(), n)
        host_t.append((time.perf_counter() - t0) * 1e6)
    same = np.array_equal(hm, mom.cpu().numpy()) and np.array_equal(hp, pts[:n, TMAX:TMAX + Fw].cpu().numpy())
    p = pts[:n, TMAX:TMAX + Fw].cpu().numpy().astype(np.int64)
    ok = (p[:, 1:] >= 0).all(-1) & (p[:, :-1] >= 0).all(-1)
    step = np.abs(p[:, 1:] - p[:, :-1]).max(-1)[ok]
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d (bench.synth_video, uint8); %d of %d (track, frame) centroids present,"
             % (n, Fw, h, w, int((p >= 0).all(-1).sum()), n * Fw),
             "# median step between consecutive centroids %d pixels (the generator's regions are redrawn per frame: longer segments than a real track's)"
             % (int(np.median(step)) if len(step) else -1),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "%-58s %6s %9s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "- alone", "/ alone")]
    for i, (name, _) in enumerate(variants):
        x, b = res[name], base_y if name.startswith("NV12") else base
        lines.append("%-58s %6d %9.1f %9.1f %9.1f %9.1f %8.2f" % (name, reps[name], med[name], min(x), max(x), med[name] - b, med[name] / b))
    lines.append("host alternative: the read-back above (%.1f us beyond the stage) + numpy centroids on the host: %.0f us (min of 3; three "
                 "bincounts per frame); integers equal to the kernel's: %s" % (med[variants[-1][0]] - base, min(host_t), same))
    lines.append("so the window with centroids and a trail of 16 costs %.2fx the window without; the host route to the centroids alone costs %.1fx"
                 % (med[variants[2][0]] / base, (med[variants[-1][0]] + min(host_t)) / base))
    emit(lines)


if __name__ == "__main__":
    launches()
