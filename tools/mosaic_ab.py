"""What the mosaic overlay costs: the new launches (mdqe_render_mosaic_u8 with uint8 and float32 frames, mdqe_render_mosaic_yuv420sp on
NV12 and P010 surfaces; mosaic on the tracks and on the background, cell 16) beside the plain painters on the same inputs
(mdqe_render_overlay_u8 / mdqe_render_overlay_yuv420sp, contour 0 and 1) and beside tools/overlay_ab.py's yardstick, a device-to-device
copy that moves the same algorithmic bytes (RGB uint8: 1 label + 3 frame bytes in, 3 out = 7 B per pixel; NV12: 1 + 1.5 + 1.5 = 4;
P010: 7): the aim is a paint within twice its copy.  One window of 15 tracks, the shipped 360p one (30 frames of 360 x 640, the label
generator of tools/overlay_ab.py).  Then, `mosaic_ab.py OUT e2e`, frames/s of a warm 120-frame 360p online_video(emit="overlay")
session with Style() against Style(mosaic="tracks") and Style(mosaic="background"), RGB pictures and NV12 surfaces.  Tables are
appended to OUT when given."""
import os, sys, statistics, time
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops
from mdqe_cvpr2023_amd.preprocess import YuvFrames
from mdqe_cvpr2023_amd.render import Style, default_palette, palette_yuv


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
    h, w, Fw, n, cell = 360, 640, 30, 15, 16
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/overlay_ab.py)
    g = torch.Generator().manual_seed(0)
    lg = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    ops.final_label_map(lg, torch.arange(n, dtype=torch.int32, device="cuda"), 4, h, w, h, w, lab, 0)
    fr8 = torch.randint(0, 256, (Fw, 3, h, w), generator=g, dtype=torch.uint8).cuda()
    fr32 = fr8.float()
    pic = torch.empty(Fw, h, w, 3, dtype=torch.uint8, device="cuda")
    pal = default_palette()
    pal_dev = pal.cuda()
    px = Fw * h * w
    act = {m: Style(mosaic=m).actions().cuda() for m in ("tracks", "background")}
    surf, out, pal_yuv = {}, {}, {}
    for fmt in ("nv12", "p010"):
        s = YuvFrames.empty(Fw, h, w, fmt=fmt, device="cuda")
        lo, hi, dt = (0, 256, torch.uint8) if fmt == "nv12" else (-32768, 32768, torch.int16)
        s.y.copy_(torch.randint(lo, hi, tuple(s.y.shape), generator=g, dtype=dt))
        s.uv.copy_(torch.randint(lo, hi, tuple(s.uv.shape), generator=g, dtype=dt))
        surf[fmt], out[fmt] = s, YuvFrames.empty(Fw, h, w, fmt=fmt, device="cuda")
        pal_yuv[fmt] = palette_yuv(pal, fmt, "bt709", False, "rgb").cuda()
    bufs = {b: (torch.randint(0, 256, (int(px * b / 2),), generator=g, dtype=torch.uint8).cuda(), torch.empty(int(px * b / 2), dtype=torch.uint8, device="cuda"))
            for b in (16.0, 7.0, 4.0)}

    def copy(b): return lambda: bufs[b][1].copy_(bufs[b][0])
    frames = {"RGB uint8": (fr8, 7.0), "RGB float32": (fr32, 16.0)}
    variants = [("D2D copy that moves %g B per pixel" % b, copy(b), b) for b in (16.0, 7.0, 4.0)]
    for kind, (fr, b) in frames.items():
        for c in (0, 1):
            variants.append(("%s plain overlay, contour %d" % (kind, c), (lambda fr=fr, c=c: ops.render_overlay(lab, fr, pal_dev, pic, 0, 128, c)), b))
        for m in act:
            variants.append(("%s mosaic %s" % (kind, m), (lambda fr=fr, m=m: ops.render_mosaic(lab, fr, pal_dev, act[m], pic, 0, 128, 1, cell)), b))
    for fmt, b in (("nv12", 4.0), ("p010", 7.0)):
        for c in (0, 1):
            variants.append(("%s plain overlay, contour %d" % (fmt.upper(), c),
                             (lambda fmt=fmt, c=c: ops.render_overlay_yuv(lab, surf[fmt], pal_yuv[fmt], out[fmt], 0, 128, c)), b))
        for m in act:
            variants.append(("%s mosaic %s" % (fmt.upper(), m),
                             (lambda fmt=fmt, m=m: ops.render_mosaic_yuv(lab, surf[fmt], pal_yuv[fmt], act[m], out[fmt], 0, 128, 1, cell)), b))
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
    flagged = float(F.max_pool2d((lab != 0).float()[:, None], cell, ceil_mode=True).mean())       # cells that hold a track pixel
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d, tight pitches, cell %d, a256 128, mosaic launches at contour 1;"
             % (n, Fw, h, w, cell),
             "# %.1f M pixels, labelled %.1f %%, cells with a track pixel %.1f %%" % (px / 1e6, 100 * float((lab != 0).float().mean()), 100 * flagged),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "%-44s %6s %9s %9s %9s %11s %8s" % ("variant", "reps", "median", "min", "max", "GB/s moved", "/ copy")]
    for name, _, b in variants:
        v = res[name]
        lines.append("%-44s %6d %9.1f %9.1f %9.1f %11.1f %8.2f" % (name, reps[name], med[name], min(v), max(v), px * b / med[name] / 1e3,
                                                                   med[name] / med["D2D copy that moves %g B per pixel" % b]))
    lines.append("(/ copy: against the copy of the same algorithmic bytes; the aim is <= 2)")
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
    feeds = {"RGB": (v.cuda(), False), "NV12": (s, True)}
    styles = {"Style()": Style(), "mosaic='tracks'": Style(mosaic="tracks"), "mosaic='background'": Style(mosaic="background")}

    def run(form, style):
        feed, surface = feeds[form]
        ov = model.online_video(emit="overlay", surface=surface, style=styles[style])
        t0 = time.perf_counter()
        n = 0
        for a in range(0, L, 30):
            n += len(ov.push(feed[a:a + 30]))
        n += len(ov.close())
        torch.cuda.synchronize()
        fps = L / (time.perf_counter() - t0)
        ov.result()                                # (sets model.last_num_tracks)
        return fps, n

    order = [(f, st) for f in feeds for st in styles]
    for key in order:
        run(*key)
    res = {key: [] for key in order}
    for r in range(7):
        for key in (order if r % 2 == 0 else order[::-1]):
            fps, n = run(*key)
            res[key].append(fps)
    lines = ["# end to end: %d frames of %d x %d (resident on the device) through online_video(emit='overlay') in pushes of 30, %d windows, tracks %d;"
             % (L, h, w, n, model.last_num_tracks),
             "# frames/s of push() .. close() with the windows on the host, 7 runs each in one process, order alternating, after one warm-up each",
             "%-8s %-22s %9s %9s %9s %12s" % ("picture", "style", "median", "min", "max", "/ Style()")]
    for key in order:
        x = res[key]
        lines.append("%-8s %-22s %9.1f %9.1f %9.1f %12.3f" % (key + (statistics.median(x), min(x), max(x),
                                                                     statistics.median(x) / statistics.median(res[(key[0], "Style()")]))))
    emit(lines)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "e2e":
        end_to_end()
    else:
        launches()
