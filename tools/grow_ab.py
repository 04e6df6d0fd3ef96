"""What the redaction margin costs: one tracker window's label + overlay stage (ops.final_label_map, then the painter) with
blur="tracks", blur_radius=8 at grow 0 / 4 / 8 / 16 / 32 -- at grow > 0 one ops.grow_labels launch (mdqe_grow_labels_u8) between the
two and the painter on the grown map, as merge.overlay_frames does it -- the same on NV12 surfaces, and the grow launch alone, on the
two windows of tools/blur_ab.py: 15 tracks x 30 frames of 360 x 640 of the bench's synthetic video, DENSE (nearly every pixel belongs to
a track: every tile is searched, but few pixels are left to grow into) and SPARSE (small tracks: most 16 x 64 tiles are copied).
Beside it the host alternative a caller has today: the label map and the frames read back into pinned memory, then the rule in numpy
(a sweep of shifted arrays over the disc; held to the kernel's bytes here).  Then, `grow_ab.py OUT e2e`, frames/s of a warm 120-frame
360p online_video(emit="overlay") session with blur="tracks" at grow 0 and, where the style has the field, at grow 8 and 32 (run the
grow=0 legs on the parent commit too: the untouched path).  One process, no retries.  Tables are appended to OUT when given."""
import os, sys, statistics, time
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops
from mdqe_cvpr2023_amd.preprocess import YuvFrames
from mdqe_cvpr2023_amd.render import Style

GROWS = (0, 4, 8, 16, 32)


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


def host_grow(labels, table, radius):
    """The rule of include/mdqe_hip.h on the host: for every offset of the disc the shifted map offers d2 * 256 + label where it grows."""
    big = np.int32(1 << 30)
    g = table != 0
    g[0] = False
    lab = labels.astype(np.int32)
    offer = np.where(g[labels], lab, big)
    best = np.full(labels.shape, big, dtype=np.int32)
    _, H, W = labels.shape
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            d2 = dy * dy + dx * dx
            if d2 > radius * radius or abs(dy) >= H or abs(dx) >= W:
                continue
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            view = best[:, y0:y1, x0:x1]
            np.minimum(view, offer[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx] + d2 * 256, out=view)
    return np.where((offer == big) & (best < big), best & 255, lab).astype(np.uint8)


def launches():
    from bench import synth_video
    h, w, Fw, n = 360, 640, 30, 15
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/blur_ab.py)
    g = torch.Generator().manual_seed(0)
    dense = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    sparse = (dense - 7.0).contiguous()                                      # the same blobs, only their peaks: small tracks
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    grown = torch.empty_like(lab)
    v = synth_video(0, Fw, seed=1).round().clamp(0, 255).to(torch.uint8)
    fr8 = v.cuda()
    out = torch.empty(Fw, h, w, 3, dtype=torch.uint8, device="cuda")
    s = YuvFrames.empty(Fw, h, w, device="cuda")                             # luma from the green plane, chroma from sub-sampled red and blue
    s.y.copy_(v[:, 1])
    s.uv.copy_(torch.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(Fw, h // 2, w))
    so = YuvFrames.empty(Fw, h, w, device="cuda")

    def stage(st, lg=dense, surface=False):
        pal = st.palette_yuv_on("cuda", *s.meta()[2:]) if surface else st.palette_on("cuda")
        act, taps, taps_c = st.actions_on("cuda"), st.taps_on("cuda"), st.taps_c_on("cuda")
        table = st.grows_on("cuda")

        def run():
            ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
            m = ops.grow_labels(lab, table, st.grow, grown) if st.grow > 0 else lab
            if surface: ops.render_blur_yuv(m, s, pal, act, taps, taps_c, so, 0, st.a256, st.contour)
            else: ops.render_blur(m, fr8, pal, act, taps, out, 0, st.a256, st.contour)
        return run

    def alone(lg, radius):
        table = Style(blur="tracks").grows_on("cuda")
        ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
        fixed = lab.clone()
        return lambda: ops.grow_labels(fixed, table, radius, grown)
    variants = [("label + blur='tracks' r 8, grow %d%s" % (gr, " (the stage as it was)" if gr == 0 else ""), stage(Style(blur="tracks", grow=gr)))
                for gr in GROWS]
    variants += [("NV12: label + blur='tracks' r 8, grow %d" % gr, stage(Style(blur="tracks", grow=gr), surface=True)) for gr in GROWS]
    variants += [("sparse: label + blur='tracks' r 8, grow %d" % gr, stage(Style(blur="tracks", grow=gr), sparse)) for gr in GROWS]
    variants += [("grow launch alone, radius %d" % r, alone(dense, r)) for r in GROWS]
    variants += [("sparse: grow launch alone, radius %d" % r, alone(sparse, r)) for r in GROWS]

    # the host alternative: read back what the picture is made of, then numpy
    pin = {k: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for k, t in (("lab", lab), ("frames", fr8))}

    def read_back(lg=sparse):
        ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
        for k, t in (("lab", lab), ("frames", fr8)):
            pin[k].copy_(t, non_blocking=True)
    variants.append(("sparse: label + read-back of map and frames", read_back))
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
    # the host's numpy pass on what was read back, held to the kernel's bytes (the sparse window, radius 8)
    table = Style(blur="tracks").grows()
    read_back()
    torch.cuda.synchronize()
    dev = ops.grow_labels(lab, table.cuda(), 8).cpu().numpy()
    share = float((dev != pin["lab"].numpy()).mean())
    host_t = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = host_grow(pin["lab"].numpy(), table.numpy(), 8)
        host_t.append((time.perf_counter() - t0) * 1e6)
    same = np.array_equal(got, dev)
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d (bench.synth_video, uint8)" % (n, Fw, h, w),
             "# dense window: %.1f %% of the pixels belong to a track, %.1f %% of the 16 x 64 tiles hold one; sparse window: %.2f %% and %.1f %%"
             % (100 * pd, 100 * td, 100 * ps, 100 * ts),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "# '- grow 0' and '/ grow 0': against the first line of the variant's own group",
             "%-58s %6s %9s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "- grow 0", "/ grow 0")]
    for i, (name, _) in enumerate(variants):
        x = res[name]
        base = med[variants[i - i % len(GROWS)][0]] if i < 3 * len(GROWS) else None
        lines.append("%-58s %6d %9.1f %9.1f %9.1f %9s %8s" % (name, reps[name], med[name], min(x), max(x),
                                                              "" if base is None else "%.1f" % (med[name] - base),
                                                              "" if base is None else "%.2f" % (med[name] / base)))
    sparse0 = med[variants[2 * len(GROWS)][0]]
    lines.append("host alternative, sparse window: the read-back above (%.1f us beyond the grow-0 stage) + numpy dilation of radius 8 on the "
                 "host: %.0f us (min of 3; a sweep of shifted int32 arrays); bytes equal to the kernel's: %s; %.2f %% of the pixels change"
                 % (med[variants[-1][0]] - sparse0, min(host_t), same, 100 * share))
    lines.append("so a margin of 8 costs %.2fx the blur stage of radius 8 on the dense window and %.2fx on the sparse one; the host route "
                 "costs %.0fx the sparse stage" % (med[variants[2][0]] / med[variants[0][0]], med[variants[2 * len(GROWS) + 2][0]] / sparse0,
                                                  (med[variants[-1][0]] + min(host_t)) / sparse0))
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
    if "grow" in Style.__dataclass_fields__:        # (the parent commit runs the first two legs only)
        kinds["Style(blur='tracks', grow=8)"] = Style(blur="tracks", grow=8)
        kinds["Style(blur='tracks', grow=32)"] = Style(blur="tracks", grow=32)
        kinds["Style(grow=8)"] = Style(grow=8)

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
