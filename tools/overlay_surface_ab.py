"""What painting onto decoder surfaces costs beside painting RGB pixels.  `overlay_surface_ab.py [OUT [launches [H W FRAMES] | e2e]]`:
1. the two paint launches alone on one tracker window of 15 tracks, 30 frames of 360 x 640, the same label map: mdqe_render_overlay_u8
   (planar uint8 RGB frames in, interleaved RGB out: 1 + 3 bytes in, 3 out per pixel) and mdqe_render_overlay_yuv420sp (NV12 surfaces at a
   tight pitch in and out: 1 + 1.5 in, 1.5 out; P010: 1 + 3 in, 3 out), contour 0 / 1 / 3, each beside a device-to-device copy that
   moves the same number of bytes and does nothing else;
2. frames/s of one warm online session in each form on the same 120-frame NV12 video of 360 x 640 (device surfaces, pushes of 30):
   emit="overlay" and emit="overlay", surface=True, with every window on the host.
Device events around >= 0.25 s of back-to-back calls (1) and the host clock around push() .. close() (2), 7 alternating passes, medians
with min and max: the method of profiles/score_overlap_ab.txt.  Tables are appended to OUT when given."""
import os, sys, statistics, time
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops
from mdqe_cvpr2023_amd.preprocess import YuvFrames
from mdqe_cvpr2023_amd.render import default_palette, palette_yuv


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


def launches():
    h, w, Fw = (int(v) for v in sys.argv[3:6]) if len(sys.argv) > 5 else (360, 640, 30)
    n = 15
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/overlay_ab.py)
    g = torch.Generator().manual_seed(0)
    lg = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    ops.final_label_map(lg, torch.arange(n, dtype=torch.int32, device="cuda"), 4, h, w, h, w, lab, 0)
    fr8 = torch.randint(0, 256, (Fw, 3, h, w), generator=g, dtype=torch.uint8).cuda()
    pic = torch.empty(Fw, h, w, 3, dtype=torch.uint8, device="cuda")
    pal = default_palette()
    pal_dev = pal.cuda()
    px = Fw * h * w
    surf, out, pal_yuv = {}, {}, {}
    for fmt in ("nv12", "p010"):
        s = YuvFrames.empty(Fw, h, w, fmt=fmt, device="cuda")
        if fmt == "nv12":
            s.y.copy_(torch.randint(0, 256, tuple(s.y.shape), generator=g, dtype=torch.uint8))
            s.uv.copy_(torch.randint(0, 256, tuple(s.uv.shape), generator=g, dtype=torch.uint8))
        else:
            s.y.copy_(torch.randint(-32768, 32768, tuple(s.y.shape), generator=g, dtype=torch.int16))
            s.uv.copy_(torch.randint(-32768, 32768, tuple(s.uv.shape), generator=g, dtype=torch.int16))
        surf[fmt], out[fmt] = s, YuvFrames.empty(Fw, h, w, fmt=fmt, device="cuda")
        pal_yuv[fmt] = palette_yuv(pal, fmt, "bt709", False, "rgb").cuda()
    bufs = {k: (torch.randint(0, 256, (int(px * b / 2),), generator=g, dtype=torch.uint8).cuda(), torch.empty(int(px * b / 2), dtype=torch.uint8, device="cuda"))
            for k, b in (("7", 7.0), ("4", 4.0))}

    def copy(k): return lambda: bufs[k][1].copy_(bufs[k][0])
    def rgb(c): return lambda: ops.render_overlay(lab, fr8, pal_dev, pic, 0, 128, c)
    def yuv(fmt, c): return lambda: ops.render_overlay_yuv(lab, surf[fmt], pal_yuv[fmt], out[fmt], 0, 128, c)
    variants = [("D2D copy that moves 7 B per pixel", copy("7"), 7.0), ("D2D copy that moves 4 B per pixel", copy("4"), 4.0)]
    for c in (0, 1, 3):
        variants += [("paint RGB  (uint8 planes -> interleaved), contour %d" % c, rgb(c), 7.0),
                     ("paint NV12 (surfaces -> surfaces), contour %d" % c, yuv("nv12", c), 4.0),
                     ("paint P010 (surfaces -> surfaces), contour %d" % c, yuv("p010", c), 7.0)]
    reps = {}
    for name, fn, _ in variants:
        for _ in range(5): fn()
        torch.cuda.synchronize()
        reps[name] = max(20, int(0.25e6 / timed(fn, 20)) + 1)
    res = {name: [] for name, _, _ in variants}
    for r in range(7):
        for name, fn, _ in (variants if r % 2 == 0 else variants[::-1]):           # alternating order
            res[name].append(timed(fn, reps[name]))
    med = {k: statistics.median(v) for k, v in res.items()}
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d, tight pitches; %.1f M pixels, labelled %.1f %%"
             % (n, Fw, h, w, px / 1e6, 100 * float((lab != 0).float().mean())),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "%-56s %6s %9s %9s %9s %12s" % ("variant", "reps", "median", "min", "max", "GB/s moved")]
    for name, _, b in variants:
        v = res[name]
        lines.append("%-56s %6d %9.1f %9.1f %9.1f %12.1f" % (name, reps[name], med[name], min(v), max(v), px * b / med[name] / 1e3))
    for c in (0, 1, 3):
        r_, n_, p_ = (med[variants[2 + 3 * (0, 1, 3).index(c) + k][0]] for k in range(3))
        lines.append("contour %d: NV12 / RGB = %.2f, P010 / RGB = %.2f; NV12 / its copy = %.2f, RGB / its copy = %.2f"
                     % (c, n_ / r_, p_ / r_, n_ / med[variants[1][0]], r_ / med[variants[0][0]]))
    emit(lines)


def end_to_end():
    from bench import synth_video
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = PRESETS["R50_ovis_360"]
    model = MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()
    L, h, w = 120, 360, 640
    v = synth_video(0, L, seed=1).round().clamp(0, 255).to(torch.uint8)
    s = YuvFrames.empty(L, h, w, device="cuda")                                # luma from the green plane, chroma from sub-sampled red and blue
    s.y.copy_(v[:, 1])
    s.uv.copy_(torch.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(L, h // 2, w))

    def run(surface):
        ov = model.online_video(emit="overlay", surface=surface)
        t0 = time.perf_counter()
        n = 0
        for a in range(0, L, 30):
            n += len(ov.push(s[a:a + 30]))
        n += len(ov.close())
        torch.cuda.synchronize()
        fps = L / (time.perf_counter() - t0)
        ov.result()                                # (sets model.last_num_tracks)
        return fps, n

    for surface in (False, True):
        run(surface)
    res = {False: [], True: []}
    for r in range(7):
        for surface in ((False, True) if r % 2 == 0 else (True, False)):
            fps, n = run(surface)
            res[surface].append(fps)
    lines = ["# end to end: %d NV12 surfaces of %d x %d (resident on the device, tight pitch) through online_video(emit='overlay') in pushes of 30,"
             % (L, h, w),
             "# %d windows, tracks %d; frames/s of push() .. close() with the windows on the host, 7 runs each, alternating, after one warm-up each"
             % (n, model.last_num_tracks),
             "%-28s %9s %9s %9s %28s" % ("form", "median", "min", "max", "kept + read back per pixel")]
    for surface, name, b in ((False, "RGB pixels (surface=False)", "3 + 3 B"), (True, "NV12 surfaces (surface=True)", "1.5 + 1.5 B")):
        x = res[surface]
        lines.append("%-28s %9.1f %9.1f %9.1f %28s" % (name, statistics.median(x), min(x), max(x), b))
    lines.append("surface / RGB = %.3f   (read-back per video: %.1f MB against %.1f MB)"
                 % (statistics.median(res[True]) / statistics.median(res[False]), L * h * w * 1.5 / 1e6, L * h * w * 3 / 1e6))
    emit(lines)


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[2] == "launches":
        launches()
    if len(sys.argv) < 3 or sys.argv[2] == "e2e":
        end_to_end()
