"""What the edge-stopping blur costs against the plain one: one tracker window's label + overlay stage (ops.final_label_map, then
ops.render_blur / ops.render_blur_yuv) with blur="tracks" and blur="background" at radius 4, 8, 16, 32, edge "bleed"
(mdqe_render_blur_u8 / _yuv420sp) against "stop" (mdqe_render_blur_within_u8 / _yuv420sp), on uint8 RGB frames and on NV12 surfaces, on
the two windows of tools/blur_ab.py: 15 tracks x 30 frames of 360 x 640, one DENSE (the tracks cover the picture: blur="tracks" makes
nearly every pixel a member, blur="background" nearly none) and one SPARSE (small tracks: most 16 x 64 tiles skip the filter with
"tracks", every tile runs it with "background").  Then, `blur_edge_ab.py OUT e2e`, frames/s of a warm 120-frame 360p
online_video(emit="overlay") session with Style(), Style(blur="tracks") and blur_edge="stop" at radius 8 and 32 (run it on the parent
commit too: it runs the first two legs there, the untouched path).  One process, no retries.  Tables are appended to OUT when given."""
import os, sys, statistics, time
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops
from mdqe_cvpr2023_amd.preprocess import YuvFrames
from mdqe_cvpr2023_amd.render import Style

RADII = (4, 8, 16, 32)


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
    from bench import synth_video
    h, w, Fw, n = 360, 640, 30, 15
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/blur_ab.py)
    g = torch.Generator().manual_seed(0)
    dense = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    sparse = (dense - 7.0).contiguous()                                      # the same blobs, only their peaks: small tracks
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    v = synth_video(0, Fw, seed=1).round().clamp(0, 255).to(torch.uint8)
    fr8 = v.cuda()
    out = torch.empty(Fw, h, w, 3, dtype=torch.uint8, device="cuda")
    s = YuvFrames.empty(Fw, h, w, device="cuda")                             # luma from the green plane, chroma from sub-sampled red and blue
    s.y.copy_(v[:, 1])
    s.uv.copy_(torch.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(Fw, h // 2, w))
    so = YuvFrames.empty(Fw, h, w, device="cuda")

    def stage(st, lg, surface):
        pal = st.palette_yuv_on("cuda", *s.meta()[2:]) if surface else st.palette_on("cuda")
        act = st.actions_on("cuda") if st.blur else None
        taps, taps_c = (st.taps_on("cuda"), st.taps_c_on("cuda")) if st.blur else (None, None)
        edge = st.blur_edge

        def run():
            ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
            if st.blur and surface: ops.render_blur_yuv(lab, s, pal, act, taps, taps_c, so, 0, st.a256, st.contour, edge=edge)
            elif st.blur: ops.render_blur(lab, fr8, pal, act, taps, out, 0, st.a256, st.contour, edge=edge)
            elif surface: ops.render_overlay_yuv(lab, s, pal, so, 0, st.a256, st.contour)
            else: ops.render_overlay(lab, fr8, pal, out, 0, st.a256, st.contour)
        return run
    variants, pairs = [], []
    for wname, lg in (("dense", dense), ("sparse", sparse)):
        for surface in (False, True):
            kind = "NV12" if surface else "RGB"
            variants.append(("%s %s: label + plain overlay" % (wname, kind), stage(Style(), lg, surface)))
            for what in ("tracks", "background"):
                for r in RADII:
                    names = []
                    for edge in ("bleed", "stop"):
                        name = "%s %s: blur='%s' r %d, %s" % (wname, kind, what, r, edge)
                        variants.append((name, stage(Style(blur=what, blur_radius=r, blur_edge=edge), lg, surface)))
                        names.append(name)
                    pairs.append((wname, kind, what, r, names))
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

    def tiles(lg):                                                            # the share of 16 x 64 tiles that hold a track pixel
        ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
        m = (lab != 0).cpu()
        t = F.max_pool2d(m.float()[:, None], (16, 64), ceil_mode=True)
        return float(t.mean()), float(m.float().mean())
    (td, pd), (ts, ps) = tiles(dense), tiles(sparse)
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d (bench.synth_video, uint8)" % (n, Fw, h, w),
             "# dense window: %.1f %% of the pixels belong to a track, %.1f %% of the 16 x 64 tiles hold one; sparse window: %.2f %% and %.1f %%"
             % (100 * pd, 100 * td, 100 * ps, 100 * ts),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "# '/ bleed': the stage with edge='stop' over the same stage with edge='bleed' (medians)",
             "%-52s %6s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "/ bleed")]
    for name, _ in variants:
        x = res[name]
        ratio = "%8.2f" % (med[name] / med[name[:-4] + "bleed"]) if name.endswith("stop") else ""
        lines.append("%-52s %6d %9.1f %9.1f %9.1f %8s" % (name, reps[name], med[name], min(x), max(x), ratio))
    lines.append("")
    lines.append("# stop / bleed of the whole stage, per radius (%s)" % ", ".join("r %d" % r for r in RADII))
    for wname in ("dense", "sparse"):
        for kind in ("RGB", "NV12"):
            for what in ("tracks", "background"):
                row = [med[nm[1]] / med[nm[0]] for (a, b, c, r, nm) in pairs if (a, b, c) == (wname, kind, what)]
                lines.append("%-36s %s" % ("%s %s blur='%s'" % (wname, kind, what), "  ".join("%5.2f" % x for x in row)))
    emit(lines)


def end_to_end():
    from bench import synth_video
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = PRESETS["R50_ovis_360"]
    model = MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()
    L, h, w = 120, 360, 640
    feed = synth_video(0, L, seed=1).round().clamp(0, 255).to(torch.uint8).cuda()
    kinds = {"Style()": Style(), "Style(blur='tracks')": Style(blur="tracks")}
    if "blur_edge" in Style.__dataclass_fields__:   # (the parent commit runs the first two legs only)
        kinds["Style(blur='tracks', blur_edge='stop')"] = Style(blur="tracks", blur_edge="stop")
        kinds["Style(blur='tracks', blur_edge='stop', r 32)"] = Style(blur="tracks", blur_edge="stop", blur_radius=32)
        kinds["Style(blur='background', blur_edge='stop')"] = Style(blur="background", blur_edge="stop")
        kinds["Style(blur='background', blur_edge='stop', r 32)"] = Style(blur="background", blur_edge="stop", blur_radius=32)

    def run(kind):
        ov = model.online_video(emit="overlay", style=kinds[kind])
        t0 = time.perf_counter()
        n = 0
        for a in range(0, L, 30):
            n += len(ov.push(feed[a:a + 30]))
        n += len(ov.close())
        torch.cuda.synchronize()
        fps = L / (time.perf_counter() - t0)
        ov.result()                                # (sets model.last_num_tracks)
        return fps, n

    order = list(kinds)
    for key in order:
        run(key)
    res = {key: [] for key in order}
    for r in range(7):
        for key in (order if r % 2 == 0 else order[::-1]):
            fps, n = run(key)
            res[key].append(fps)
    lines = ["# end to end: %d frames of %d x %d (resident on the device) through online_video(emit='overlay') in pushes of 30, %d windows, tracks %d;"
             % (L, h, w, n, model.last_num_tracks),
             "# frames/s of push() .. close() with the windows on the host, 7 runs each in one process, order alternating, after one warm-up each",
             "%-52s %9s %9s %9s %12s" % ("session", "median", "min", "max", "/ Style()")]
    for key in order:
        x = res[key]
        lines.append("%-52s %9.1f %9.1f %9.1f %12.3f" % (key, statistics.median(x), min(x), max(x),
                                                         statistics.median(x) / statistics.median(res["Style()"])))
    emit(lines)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "e2e":
        end_to_end()
    else:
        launches()
