"""What per-track crops cost: one tracker window's label stage (ops.final_label_map with its geometry table) alone and with the crops
launch behind it (mdqe_track_crops_u8 on uint8 RGB frames, mdqe_track_crops_yuv420sp on NV12 surfaces; 128 x 64 chips plain, padded,
cut out, every second frame; 32 x 32 chips; a 1 x 1 chip, the wave form) -- the comparison is the same window without crops.  One
window of 15 tracks, the shipped 360p one (30 frames of 360 x 640 of the bench's synthetic video, the label generator of
tools/overlay_ab.py).  Beside it the host alternative a caller has today: the label map, the table and the frames read back into pinned
memory, then the crops in numpy (integral images: the same integers, held to the kernel's bytes here).  Then, `crops_ab.py OUT e2e`,
frames/s of a warm 120-frame 360p online_video(emit="masks") session without and with crops=.  Tables are appended to OUT when given."""
import os, sys, statistics, time
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops
from mdqe_cvpr2023_amd.preprocess import YuvFrames
from mdqe_cvpr2023_amd.render import Crops


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


def host_crops(frames, labels, geom, n, size, pad256=0, every=1):
    """The rule of include/mdqe_hip.h on the host for uint8 frames at the output size, without cutout: per frame one integral image,
    per chip four gathers."""
    Fw, Ho, Wo = labels.shape
    Sh, Sw = size
    taken = list(range(0, Fw, every))
    out = np.zeros((n, len(taken), Sh, Sw, 3), dtype=np.uint8)
    i, j = np.arange(Sh, dtype=np.int64), np.arange(Sw, dtype=np.int64)
    for t, f in enumerate(taken):
        I = np.zeros((Ho + 1, Wo + 1, 3), dtype=np.int64)
        I[1:, 1:] = np.moveaxis(frames[f], 0, -1).astype(np.int64).cumsum(0).cumsum(1)
        for k in range(n):
            area, x0, y0, x1, y1 = (int(v) for v in geom[k, f])
            if not (area >= 1 and 0 <= x0 <= x1 < Wo and 0 <= y0 <= y1 < Ho):
                continue
            px, py = ((x1 - x0 + 1) * pad256 + 128) >> 8, ((y1 - y0 + 1) * pad256 + 128) >> 8
            X0, X1, Y0, Y1 = max(x0 - px, 0), min(x1 + px, Wo - 1), max(y0 - py, 0), min(y1 + py, Ho - 1)
            cw, ch = X1 - X0 + 1, Y1 - Y0 + 1
            Ya, Yb = Y0 + (i * ch) // Sh, Y0 + ((i + 1) * ch + Sh - 1) // Sh
            Xa, Xb = X0 + (j * cw) // Sw, X0 + ((j + 1) * cw + Sw - 1) // Sw
            s = I[Yb][:, Xb] - I[Ya][:, Xb] - I[Yb][:, Xa] + I[Ya][:, Xa]
            m = ((Yb - Ya)[:, None] * (Xb - Xa)[None, :])[:, :, None]
            out[k, t] = (s + m // 2) // m
    return out


def launches():
    from bench import synth_video
    h, w, Fw, n = 360, 640, 30, 15
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/overlay_ab.py)
    g = torch.Generator().manual_seed(0)
    lg = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    geom = torch.empty(n * Fw, 5, dtype=torch.int32, device="cuda")
    v = synth_video(0, Fw, seed=1).round().clamp(0, 255).to(torch.uint8)
    fr8 = v.cuda()
    s = YuvFrames.empty(Fw, h, w, device="cuda")                             # luma from the green plane, chroma from sub-sampled red and blue
    s.y.copy_(v[:, 1])
    s.uv.copy_(torch.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(Fw, h // 2, w))

    def stage(spec=None, src=fr8):
        def run():
            ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0, geom=geom)
            if spec is not None:
                fn = ops.track_crops if torch.is_tensor(src) else ops.track_crops_yuv
                fn(lab, src, geom, n, spec.size, bufs[spec][0], 0, bufs[spec][1], 0, spec.every, spec.pad256, spec.min_area, spec.cutout, spec.fill)
        return run
    specs = {"128 x 64": Crops(), "128 x 64, pad 0.125": Crops(pad=0.125), "128 x 64, cutout": Crops(cutout=True),
             "128 x 64, every 2": Crops(every=2), "32 x 32": Crops(size=(32, 32)), "1 x 1 (wave form)": Crops(size=(1, 1))}
    bufs = {sp: (torch.empty((n, sp.count(Fw)) + sp.size + (3,), dtype=torch.uint8, device="cuda"),
                 torch.empty((n, sp.count(Fw), 4), dtype=torch.int32, device="cuda")) for sp in specs.values()}
    variants = [("label stage alone (the window without crops)", stage())]
    variants += [("label stage + crops, RGB uint8, " + k, stage(sp)) for k, sp in specs.items()]
    variants += [("label stage + crops, NV12, " + k, stage(sp, s)) for k, sp in list(specs.items())[:1]]

    # the host alternative: read back what the crops are made of, then numpy
    pin = {k: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for k, t in (("lab", lab), ("geom", geom), ("frames", fr8))}

    def read_back():
        ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0, geom=geom)
        for k, t in (("lab", lab), ("geom", geom), ("frames", fr8)):
            pin[k].copy_(t, non_blocking=True)
    variants.append(("label stage + read-back of map, table and frames", read_back))
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
    # the host's numpy pass on what was read back, held to the kernel's bytes
    stage(specs["128 x 64, pad 0.125"])()
    read_back()
    torch.cuda.synchronize()
    host_t = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = host_crops(pin["frames"].numpy(), pin["lab"].numpy(), pin["geom"].numpy().reshape(n, Fw, 5), n, (128, 64), pad256=32)
        host_t.append((time.perf_counter() - t0) * 1e6)
    same = np.array_equal(got, bufs[specs["128 x 64, pad 0.125"]][0].cpu().numpy())
    live = int((geom.view(n, Fw, 5)[:, :, 0] > 0).sum())
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d (bench.synth_video, uint8); %d of %d (track, frame) rows live"
             % (n, Fw, h, w, live, n * Fw),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "%-58s %6s %9s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "- alone", "/ alone")]
    for name, _ in variants:
        x = res[name]
        lines.append("%-58s %6d %9.1f %9.1f %9.1f %9.1f %8.2f" % (name, reps[name], med[name], min(x), max(x), med[name] - base, med[name] / base))
    lines.append("host alternative: the read-back above (%.1f us beyond the stage) + numpy crops of 128 x 64, pad 0.125 on the host: %.0f us "
                 "(min of 3; integral images, no cutout); bytes equal to the kernel's: %s"
                 % (med[variants[-1][0]] - base, min(host_t), same))
    lines.append("so the window with crops on the device costs %.2fx the window without; the host route costs %.1fx"
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
    kinds = {"no crops": None, "Crops()": Crops(), "Crops(cutout=True, pad=0.125)": Crops(cutout=True, pad=0.125), "Crops(every=5)": Crops(every=5)}

    def run(kind):
        ov = model.online_video(emit="masks", crops=kinds[kind])
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
    lines = ["# end to end: %d frames of %d x %d (resident on the device) through online_video(emit='masks') in pushes of 30, %d windows, tracks %d;"
             % (L, h, w, n, model.last_num_tracks),
             "# frames/s of push() .. close() with the windows on the host, 7 runs each in one process, order alternating, after one warm-up each",
             "%-34s %9s %9s %9s %12s" % ("session", "median", "min", "max", "/ no crops")]
    for key in order:
        x = res[key]
        lines.append("%-34s %9.1f %9.1f %9.1f %12.3f" % (key, statistics.median(x), min(x), max(x),
                                                         statistics.median(x) / statistics.median(res["no crops"])))
    emit(lines)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "e2e":
        end_to_end()
    else:
        launches()
