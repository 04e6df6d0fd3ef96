"""What the blur redaction costs: one tracker window's label + overlay stage (ops.final_label_map, then the painter) with the plain painter,
with the mosaic painter (mosaic="tracks", cell 16: the sibling on the same box) and with the blur painter (mdqe_render_blur_u8 on uint8
RGB frames: blur="tracks" at radius 4, 8, 16, 32, blur="background" at radius 16; mdqe_render_blur_yuv420sp on NV12 surfaces at radius
16), and the same on a SPARSE window whose tracks are small, where most 16 x 64 tiles skip the filter.  One window of 15 tracks, the
shipped 360p one (30 frames of 360 x 640 of the bench's synthetic video, the label generator of tools/overlay_ab.py).  Beside it the
host alternative a caller has today: the label map and the frames read back into pinned memory, then the rule in numpy (shifted sums;
held to the kernel's bytes here).  Then, `blur_ab.py OUT e2e`, frames/s of a warm 120-frame 360p online_video(emit="overlay") session
without and with the style.  Tables are appended to OUT when given."""
import os, sys, statistics, time
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops
from mdqe_cvpr2023_amd.preprocess import YuvFrames
from mdqe_cvpr2023_amd.render import Style, blur_taps


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


def host_blur(frames, labels, action, taps):
    """The rule of include/mdqe_hip.h on the host for uint8 frames at the output size, keep and blur only: shifted sums over an
    edge-padded copy, rows then columns."""
    w = [int(v) for v in taps]
    R = len(w) - 1
    s = np.moveaxis(frames, 1, -1).astype(np.int32)

    def one(t, axis, add, shift):
        n = t.shape[axis]
        pad = [(0, 0)] * t.ndim
        pad[axis] = (R, R)
        e = np.pad(t, pad, mode="edge")
        acc = np.zeros_like(t)
        for d in range(-R, R + 1):
            acc += w[abs(d)] * np.take(e, np.arange(R + d, R + d + n), axis=axis)
        return (acc + add) >> shift
    b = one(one(s, 2, 128, 8), 1, 32768, 16)
    return np.where((action[labels] == 3)[..., None], b, s).astype(np.uint8)


def launches():
    from bench import synth_video
    h, w, Fw, n = 360, 640, 30, 15
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/overlay_ab.py)
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

    def stage(st, lg=dense, surface=False):
        pal = st.palette_yuv_on("cuda", *s.meta()[2:]) if surface else st.palette_on("cuda")
        act = st.actions_on("cuda") if st.mosaic or st.blur else None
        taps, taps_c = (st.taps_on("cuda"), st.taps_c_on("cuda")) if st.blur else (None, None)

        def run():
            ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
            if st.blur and surface: ops.render_blur_yuv(lab, s, pal, act, taps, taps_c, so, 0, st.a256, st.contour)
            elif st.blur: ops.render_blur(lab, fr8, pal, act, taps, out, 0, st.a256, st.contour)
            elif st.mosaic: ops.render_mosaic(lab, fr8, pal, act, out, 0, st.a256, st.contour, st.cell)
            elif surface: ops.render_overlay_yuv(lab, s, pal, so, 0, st.a256, st.contour)
            else: ops.render_overlay(lab, fr8, pal, out, 0, st.a256, st.contour)
        return run
    variants = [("label + plain overlay, RGB uint8 (the stage alone)", stage(Style())),
                ("label + mosaic='tracks', cell 16", stage(Style(mosaic="tracks", cell=16)))]
    variants += [("label + blur='tracks', radius %d" % r, stage(Style(blur="tracks", blur_radius=r))) for r in (4, 8, 16, 32)]
    variants += [("label + blur='background', radius 16", stage(Style(blur="background", blur_radius=16))),
                 ("label + plain overlay, NV12", stage(Style(), surface=True)),
                 ("label + blur='tracks', radius 16, NV12", stage(Style(blur="tracks", blur_radius=16), surface=True)),
                 ("label + blur='background', radius 16, NV12", stage(Style(blur="background", blur_radius=16), surface=True)),
                 ("sparse: label + plain overlay", stage(Style(), sparse)),
                 ("sparse: label + blur='tracks', radius 16", stage(Style(blur="tracks", blur_radius=16), sparse)),
                 ("sparse: label + blur='tracks', radius 32", stage(Style(blur="tracks", blur_radius=32), sparse))]

    # the host alternative: read back what the picture is made of, then numpy
    pin = {k: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for k, t in (("lab", lab), ("frames", fr8))}

    def read_back():
        ops.final_label_map(dense, idx, 4, h, w, h, w, lab, 0)
        for k, t in (("lab", lab), ("frames", fr8)):
            pin[k].copy_(t, non_blocking=True)
    variants.append(("label + read-back of map and frames", read_back))
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

    def tiles(lg):                                                            # the share of 16 x 64 tiles that hold a track pixel
        ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
        m = (lab != 0).cpu()
        t = F.max_pool2d(m.float()[:, None], (16, 64), ceil_mode=True)
        return float(t.mean()), float(m.float().mean())
    (td, pd), (ts, ps) = tiles(dense), tiles(sparse)
    # the host's numpy pass on what was read back, held to the kernel's bytes (radius 8, blur="tracks", untinted: keep and blur only)
    st = Style(blur="tracks", blur_radius=8)
    stage(st)()
    read_back()
    torch.cuda.synchronize()
    host_t = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = host_blur(pin["frames"].numpy(), pin["lab"].numpy(), st.actions().numpy(), blur_taps(8).tolist())
        host_t.append((time.perf_counter() - t0) * 1e6)
    same = np.array_equal(got, out.cpu().numpy())
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d (bench.synth_video, uint8)" % (n, Fw, h, w),
             "# dense window: %.1f %% of the pixels belong to a track, %.1f %% of the 16 x 64 tiles hold one; sparse window: %.2f %% and %.1f %%"
             % (100 * pd, 100 * td, 100 * ps, 100 * ts),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "%-58s %6s %9s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "- alone", "/ alone")]
    for name, _ in variants:
        x = res[name]
        lines.append("%-58s %6d %9.1f %9.1f %9.1f %9.1f %8.2f" % (name, reps[name], med[name], min(x), max(x), med[name] - base, med[name] / base))
    lines.append("host alternative: the read-back above (%.1f us beyond the stage) + numpy blur of radius 8 on the host: %.0f us "
                 "(min of 3; shifted sums in int32); bytes equal to the kernel's: %s"
                 % (med[variants[-1][0]] - base, min(host_t), same))
    lines.append("so the stage with blur='tracks' at radius 8 costs %.2fx the plain stage on the device; the host route costs %.1fx"
                 % (med[variants[3][0]] / base, (med[variants[-1][0]] + min(host_t)) / base))
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
    kinds = {"Style()": Style(), "Style(mosaic='tracks')": Style(mosaic="tracks"), "Style(blur='tracks')": Style(blur="tracks"),
             "Style(blur='tracks', blur_radius=32)": Style(blur="tracks", blur_radius=32),
             "Style(blur='background', blur_radius=32)": Style(blur="background", blur_radius=32)}

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
