"""What the annotation pass costs: the new launches (mdqe_annotate_u8 on an RGB picture, mdqe_annotate_yuv420sp on NV12 and P010
surfaces; box 2 with captions at text scale 1 and 2, and boxes alone) beside the plain painter launch that precedes them on the same
inputs (mdqe_render_overlay_u8 / mdqe_render_overlay_yuv420sp, contour 1) -- the yardstick: the pass should cost less than the painter
it follows, since it touches a small share of the tiles and a painter touches every pixel.  One window of 15 tracks, the shipped 360p
one (30 frames of 360 x 640, the label generator of tools/overlay_ab.py; the geometry table is the one ops.final_label_map writes for
it).  Then, `annotate_ab.py OUT e2e`, frames/s of a warm 120-frame 360p online_video(emit="overlay") session with Style() against
Style(box=2, caption="id+class+score"), RGB pictures and NV12 surfaces.  Tables are appended to OUT when given."""
import os, sys, statistics, time
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops, render
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
    h, w, Fw, n = 360, 640, 30, 15
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/overlay_ab.py)
    g = torch.Generator().manual_seed(0)
    lg = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    geom = ops.final_label_map(lg, torch.arange(n, dtype=torch.int32, device="cuda"), 4, h, w, h, w, lab, 0, geom=True)[1]
    fr8 = torch.randint(0, 256, (Fw, 3, h, w), generator=g, dtype=torch.uint8).cuda()
    pal = default_palette()
    ink = render.ink(pal)
    cls = torch.rand(n, 25, generator=g)
    text = render.captions(Style(caption="id+class+score"), cls, n)
    text_dev, font = text.cuda(), render.default_font().cuda()
    pal_dev, ink_dev = pal.cuda(), ink.cuda()
    pic = torch.empty(Fw, h, w, 3, dtype=torch.uint8, device="cuda")
    ops.render_overlay(lab, fr8, pal_dev, pic, 0, 128, 1)
    surf, out, pal_yuv, ink_yuv = {}, {}, {}, {}
    for fmt in ("nv12", "p010"):
        s = YuvFrames.empty(Fw, h, w, fmt=fmt, device="cuda")
        lo, hi, dt = (0, 256, torch.uint8) if fmt == "nv12" else (-32768, 32768, torch.int16)
        s.y.copy_(torch.randint(lo, hi, tuple(s.y.shape), generator=g, dtype=dt))
        s.uv.copy_(torch.randint(lo, hi, tuple(s.uv.shape), generator=g, dtype=dt))
        surf[fmt], out[fmt] = s, YuvFrames.empty(Fw, h, w, fmt=fmt, device="cuda")
        pal_yuv[fmt] = palette_yuv(pal, fmt, "bt709", False, "rgb").cuda()
        ink_yuv[fmt] = palette_yuv(ink, fmt, "bt709", False, "rgb").cuda()
        ops.render_overlay_yuv(lab, s, pal_yuv[fmt], out[fmt], 0, 128, 1)
    cases = (("box 2, captions at scale 1", 2, 1, True), ("box 2, captions at scale 2", 2, 2, True), ("box 2 alone", 2, 1, False))
    # what a launch draws: the pixels one call changes on the freshly painted RGB picture
    share = {}
    for name, box, scale, caps in cases:
        fresh = pic.clone()
        ops.annotate(fresh, geom, n, pal_dev, ink_dev, text_dev if caps else None, font, 0, box, scale, 0)
        share[name] = 100 * float((fresh != pic).any(-1).float().mean())
    variants = [("RGB uint8 plain overlay, contour 1", lambda: ops.render_overlay(lab, fr8, pal_dev, pic, 0, 128, 1), "RGB uint8")]
    for name, box, scale, caps in cases:
        variants.append(("RGB uint8 annotate, " + name, (lambda box=box, scale=scale, caps=caps:
                                                          ops.annotate(pic, geom, n, pal_dev, ink_dev, text_dev if caps else None, font, 0, box, scale, 0)), "RGB uint8"))
    for fmt in ("nv12", "p010"):
        variants.append(("%s plain overlay, contour 1" % fmt.upper(), (lambda fmt=fmt: ops.render_overlay_yuv(lab, surf[fmt], pal_yuv[fmt], out[fmt], 0, 128, 1)),
                         fmt.upper()))
        for name, box, scale, caps in cases:
            variants.append(("%s annotate, %s" % (fmt.upper(), name),
                             (lambda fmt=fmt, box=box, scale=scale, caps=caps:
                              ops.annotate_yuv(out[fmt], geom, n, pal_yuv[fmt], ink_yuv[fmt], text_dev if caps else None, font, 0, box, scale, 0)), fmt.upper()))
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
    live = int((geom.view(n, Fw, 5)[:, :, 0] > 0).sum())
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d, tight pitches; %d of %d (track, frame) rows live; captions 'id class score%%'"
             % (n, Fw, h, w, live, n * Fw),
             "# of %d..%d characters; pixels one call changes on the painted RGB picture: %s"
             % (min(len(bytes(r.tolist()).split(b"\0")[0]) for r in text[1:n + 1]), max(len(bytes(r.tolist()).split(b"\0")[0]) for r in text[1:n + 1]),
                ", ".join("%s %.2f %%" % (k, v) for k, v in share.items())),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "%-48s %6s %9s %9s %9s %10s" % ("variant", "reps", "median", "min", "max", "/ painter")]
    for name, _, kind in variants:
        v = res[name]
        painter = med[[k for k, _, q in variants if q == kind][0]]
        lines.append("%-48s %6d %9.1f %9.1f %9.1f %10.2f" % (name, reps[name], med[name], min(v), max(v), med[name] / painter))
    lines.append("(/ painter: against the plain painter launch of the same picture kind; the expectation is < 1)")
    for kind in ("RGB uint8", "NV12", "P010"):
        ratios = [med[k] / med[[k for k, _, q in variants if q == kind][0]] for k, _, q in variants if q == kind][1:]
        lines.append("%s: the pass costs %s than the painter it follows (%s)" % (
            kind, "less" if max(ratios) < 1 else "MORE" if min(ratios) >= 1 else "less in some cases and MORE in others",
            " / ".join("%.2f" % r for r in ratios)))
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
    styles = {"Style()": Style(), "box=2, caption='id+class+score'": Style(box=2, caption="id+class+score"), "box=2": Style(box=2)}

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
             "%-8s %-34s %9s %9s %9s %12s" % ("picture", "style", "median", "min", "max", "/ Style()")]
    for key in order:
        x = res[key]
        lines.append("%-8s %-34s %9.1f %9.1f %9.1f %12.3f" % (key + (statistics.median(x), min(x), max(x),
                                                                     statistics.median(x) / statistics.median(res[(key[0], "Style()")]))))
    emit(lines)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "e2e":
        end_to_end()
    else:
        launches()
