"""What the soft matte and the background replacement cost: one tracker window's label + overlay stage (ops.final_label_map, then the
painter) with the plain painter, and with a replace style -- the label map, ops.final_matte (one more sweep of the same logits) and
ops.render_replace (mdqe_render_replace_u8 on uint8 RGB frames) -- in each mode with a colour and with a picture backdrop, and the same
on NV12 surfaces (mdqe_render_replace_yuv420sp, a colour and a surface backdrop) beside the plain surface painter; the matte
sweep alone beside the label sweep alone; and the host alternative a caller has today: label map, frames and the window's logits read
back into pinned memory, then the matte and the blend in numpy (held to the kernel's bytes within the matte's one level).  One window
of 15 tracks, the shipped 360p one (30 frames of 360 x 640 of the bench's synthetic video, the label generator of tools/overlay_ab.py).
Then, `replace_ab.py OUT e2e`, frames/s of a warm 120-frame 360p online_video(emit="overlay") session with Style() and with
Style(replace="background") (run the Style() leg on the parent commit too: the untouched path).  Tables are appended to OUT when given."""
import os, sys, statistics, time
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops
from mdqe_cvpr2023_amd.preprocess import YuvFrames
from mdqe_cvpr2023_amd.render import Style


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


def host_replace(logits, frames, labels, h, w, backdrop):
    """replace="background" with alpha = 0 on the host from what was read back: x4 aligned bilinear of every track's logits (the closed
    form of csrc/final_mask.h in float32 numpy, output size = frame size), max over the tracks, sigmoid, level, blend."""
    n, Fw, Hm, Wm = logits.shape
    def taps(size, cells):
        s = np.arange(size)
        f = np.maximum(s - 2, 0) / 4.0
        i0 = np.minimum(f.astype(np.int64), cells - 1)
        return i0, np.minimum(i0 + 1, cells - 1), (f - i0).astype(np.float32)
    y0, y1, ly = taps(h, Hm)
    x0, x1, lx = taps(w, Wm)
    vmax = np.full((Fw, h, w), -np.inf, dtype=np.float32)
    for k in range(n):
        m = logits[k]
        top = m[:, y0][:, :, x0] * (1 - lx) + m[:, y0][:, :, x1] * lx
        bot = m[:, y1][:, :, x0] * (1 - lx) + m[:, y1][:, :, x1] * lx
        np.maximum(vmax, top * (1 - ly)[None, :, None] + bot * ly[None, :, None], out=vmax)
    a = np.rint(255.0 / (1.0 + np.exp(-vmax))).astype(np.int32)
    mat = np.where(labels != 0, np.maximum(a, 128), np.minimum(a, 127))
    s = np.moveaxis(frames, 1, -1).astype(np.int32)
    wt = mat[..., None]
    return ((s * wt + backdrop.astype(np.int32) * (255 - wt) + 127) // 255).astype(np.uint8), mat.astype(np.uint8)


def launches():
    from bench import synth_video
    h, w, Fw, n = 360, 640, 30, 15
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/overlay_ab.py)
    g = torch.Generator().manual_seed(0)
    dense = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    mat = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    v = synth_video(0, Fw, seed=1).round().clamp(0, 255).to(torch.uint8)
    fr8 = v.cuda()
    out = torch.empty(Fw, h, w, 3, dtype=torch.uint8, device="cuda")
    picture = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)

    s = YuvFrames.empty(Fw, h, w, device="cuda")                             # luma from the green plane, chroma from sub-sampled red and blue
    s.y.copy_(v[:, 1])
    s.uv.copy_(torch.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(Fw, h // 2, w))
    so = YuvFrames.empty(Fw, h, w, device="cuda")
    sback = s[7:8].clone()

    def stage(st, surface=False):
        pal = st.palette_yuv_on("cuda", *s.meta()[2:]) if surface else st.palette_on("cuda")
        act = st.actions_on("cuda") if st.replace else None
        take = st.takes_on("cuda") if st.replace else None
        back = None if not st.replace else st.backdrop_yuv_on("cuda", *s.meta()[2:]) if surface else st.backdrop_on("cuda")

        def run():
            ops.final_label_map(dense, idx, 4, h, w, h, w, lab, 0)
            if st.replace:
                ops.final_matte(dense, idx, 4, h, w, h, w, mat, 0, take, st.matte_gain)
                if surface: ops.render_replace_yuv(lab, s, pal, act, mat, back, so, 0, st.a256, st.contour, st.replace)
                else: ops.render_replace(lab, fr8, pal, act, mat, back, out, 0, st.a256, st.contour, st.replace)
            elif surface: ops.render_overlay_yuv(lab, s, pal, so, 0, st.a256, st.contour)
            else: ops.render_overlay(lab, fr8, pal, out, 0, st.a256, st.contour)
        return run
    variants = [("label + plain overlay, RGB uint8 (the stage alone)", stage(Style()))]
    for mode in ("background", "tracks"):
        variants += [("label + matte + replace='%s', colour" % mode, stage(Style(replace=mode))),
                     ("label + matte + replace='%s', picture" % mode, stage(Style(replace=mode, backdrop=picture)))]
    variants += [("label + plain overlay, NV12", stage(Style(), surface=True)),
                 ("label + matte + replace='background', colour, NV12", stage(Style(replace="background"), surface=True)),
                 ("label + matte + replace='background', surface, NV12", stage(Style(replace="background", backdrop=sback), surface=True)),
                 ("label + matte + replace='tracks', colour, NV12", stage(Style(replace="tracks"), surface=True))]
    bg = Style(replace="background")
    variants += [("ops.final_label_map alone", lambda: ops.final_label_map(dense, idx, 4, h, w, h, w, lab, 0)),
                 ("ops.final_matte alone", lambda: ops.final_matte(dense, idx, 4, h, w, h, w, mat, 0, None, 1.0)),
                 ("ops.render_overlay alone", lambda: ops.render_overlay(lab, fr8, bg.palette_on("cuda"), out, 0, 128, 1))]
    variants.append(("ops.render_replace alone, colour",
                     lambda: ops.render_replace(lab, fr8, bg.palette_on("cuda"), bg.actions_on("cuda"), mat, bg.backdrop_on("cuda"), out, 0, 128, 1)))

    # the host alternative: read back what the picture is made of, then numpy
    pin = {k: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for k, t in (("lab", lab), ("frames", fr8), ("logits", dense))}

    def read_back():
        ops.final_label_map(dense, idx, 4, h, w, h, w, lab, 0)
        for k, t in (("lab", lab), ("frames", fr8), ("logits", dense)):
            pin[k].copy_(t, non_blocking=True)
    variants.append(("label + read-back of map, frames and logits", read_back))
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
    base = med[variants[0][0]]
    # the host's numpy pass on what was read back (replace="background", alpha 0, no contour: the matte and the blend only)
    st = Style(replace="background", alpha=0, contour=0)
    stage(st)()
    read_back()
    torch.cuda.synchronize()
    host_t = []
    for _ in range(3):
        t0 = time.perf_counter()
        got, hmat = host_replace(pin["logits"].numpy(), pin["frames"].numpy(), pin["lab"].numpy(), h, w, np.array(st.backdrop, dtype=np.uint8))
        host_t.append((time.perf_counter() - t0) * 1e6)
    dm = np.abs(hmat.astype(np.int32) - mat.cpu().numpy().astype(np.int32))
    dp = np.abs(got.astype(np.int32) - out.cpu().numpy().astype(np.int32))
    share = float(((mat >= 128) & (mat < 255)).float().mean()), float(((mat > 0) & (mat < 128)).float().mean())
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d (bench.synth_video, uint8)" % (n, Fw, h, w),
             "# matte of all tracks, gain 1: %.1f %% of the pixels in 128..254, %.1f %% in 1..127 (the soft edge)" % (100 * share[0], 100 * share[1]),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "%-58s %6s %9s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "- alone", "/ alone")]
    for name, _ in variants:
        x = res[name]
        lines.append("%-58s %6d %9.1f %9.1f %9.1f %9.1f %8.2f" % (name, reps[name], med[name], min(x), max(x), med[name] - base, med[name] / base))
    lines.append("host alternative: the read-back above (%.1f us beyond the stage) + numpy matte and blend on the host: %.0f us (min of 3; "
                 "float32); against the kernels: matte differs by at most %d level(s) on %.4f %% of the pixels, the picture by at most %d"
                 % (med[variants[-1][0]] - base, min(host_t), int(dm.max()), 100 * float((dm != 0).mean()), int(dp.max())))
    lines.append("so the stage with replace='background' (colour) costs %.2fx the plain stage on the device; the host route costs %.0fx"
                 % (med[variants[1][0]] / base, (med[variants[-1][0]] + min(host_t)) / base))
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
    kinds = {"Style()": Style()}
    if "replace" in Style.__dataclass_fields__:     # (the parent commit runs the first leg only)
        kinds["Style(replace='background')"] = Style(replace="background")
        kinds["Style(replace='tracks')"] = Style(replace="tracks")

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
             "%-44s %9s %9s %9s %12s" % ("session", "median", "min", "max", "/ Style()")]
    for key in order:
        x = res[key]
        lines.append("%-44s %9.1f %9.1f %9.1f %12.3f" % (key, statistics.median(x), min(x), max(x),
                                                         statistics.median(x) / statistics.median(res["Style()"])))
    emit(lines)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "e2e":
        end_to_end()
    else:
        launches()
