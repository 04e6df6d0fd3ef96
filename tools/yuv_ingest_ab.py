"""What taking decoder surfaces as input costs.  `yuv_ingest_ab.py [OUT]`, one process:
1. the conversion launch (mdqe_yuv420sp_to_rgb_u8: NV12 and P010 -> planar uint8 RGB) on 30 surfaces of 1080 x 1920 (pitch 2048 samples,
   chroma at row 1088) and of 360 x 640 (pitch 640, chroma at row 360), beside
   - a device-to-device copy of a uint8 tensor of 2.25 bytes per pixel (NV12: 1.5 B in + 3 B out = the same 4.5 B per pixel of traffic;
     P010 moves 6 B per pixel: a copy of 3 B per pixel) with nothing else to do, the yardstick: the aim is at most twice that copy;
   - what a user does today: the torch-op composition that produces the same bits (slice, widen, replicate the chroma, multiply, shift,
     clamp, stack), checked equal to the kernel's output before anything is timed;
2. end to end: frames/s of a 120-frame 360p video through online_video in pushes of 30, fed as NV12 surfaces on the device against the
   same frames as uint8 RGB tensors on the device.
Tables are appended to OUT when given."""
import os, sys, statistics, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd.preprocess import YUV_COEFFS, YuvFrames, yuv_to_rgb


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


def torch_ops(s):
    """The same bits from torch ops on the planes' device: what a user of the RGB-only interface writes today."""
    n, H, W = len(s), s.height, s.width
    yo, co, cy, rv, gu, gv, bu = YUV_COEFFS[(s.fmt, s.matrix, s.full_range)]
    ch, cw = (H + 1) // 2, (W + 1) // 2

    def samples(t):
        v = t.to(torch.int32)
        return v if s.fmt == "nv12" else (v & 0xFFFF) >> 6
    y = (samples(s.y[:, :H, :W]) - yo) * cy
    c = samples(s.uv[:, :ch, :2 * cw]).reshape(n, ch, cw, 2) - co
    c = c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W]
    u, v = c[..., 0], c[..., 1]
    planes = [y + rv * v, y + gu * u + gv * v, y + bu * u]
    return torch.stack([((p + 32768) >> 16).clamp(0, 255) for p in planes], 1).to(torch.uint8)


def surfaces(n, H, W, pitch, crow, fmt, seed):
    g = torch.Generator().manual_seed(seed)
    rows = crow + (H + 1) // 2
    if fmt == "nv12":
        buf = torch.randint(0, 256, (n, rows, pitch), generator=g, dtype=torch.uint8)
    else:
        buf = torch.randint(-32768, 32768, (n, rows, pitch), generator=g, dtype=torch.int16)
    return YuvFrames.from_surface(buf.cuda(), H, W, crow, fmt=fmt)


def launches():
    n = 30
    lines = []
    for H, W, pitch, crow in ((1080, 1920, 2048, 1088), (360, 640, 640, 360)):
        px = n * H * W
        g = torch.Generator().manual_seed(1)
        variants, moved = [], {}
        for mult, tag in ((2.25, "2.25 B per pixel (moves 4.5: NV12's traffic)"), (3.0, "3 B per pixel (moves 6: P010's traffic)")):
            src = torch.randint(0, 256, (int(px * mult),), generator=g, dtype=torch.uint8).cuda()
            dst = torch.empty_like(src)
            variants.append(("D2D copy, " + tag, (lambda s=src, d=dst: d.copy_(s))))
            moved[variants[-1][0]] = 2 * int(px * mult)
        out = torch.empty(n, 3, H, W, dtype=torch.uint8, device="cuda")
        for fmt in ("nv12", "p010"):
            s = surfaces(n, H, W, pitch, crow, fmt, seed=2)
            assert torch.equal(yuv_to_rgb(s), torch_ops(s))
            variants.append(("kernel %s" % fmt, (lambda s=s: yuv_to_rgb(s, out=out))))
            moved[variants[-1][0]] = px * (4.5 if fmt == "nv12" else 6.0)
            variants.append(("torch ops %s" % fmt, (lambda s=s: torch_ops(s))))
            moved[variants[-1][0]] = moved["kernel %s" % fmt]
        reps = {}
        for name, fn in variants:
            for _ in range(3): fn()                                             # shapes warmed before timing
            torch.cuda.synchronize()
            reps[name] = max(5, int(0.2e6 / timed(fn, 5)) + 1)
        res = {name: [] for name, _ in variants}
        for r in range(7):
            for name, fn in (variants if r % 2 == 0 else variants[::-1]):       # alternating order
                res[name].append(timed(fn, reps[name]))
        med = {k: statistics.median(v) for k, v in res.items()}
        lines += ["# %d surfaces of %d x %d, pitch %d samples, chroma at row %d; %.1f M pixels" % (n, H, W, pitch, crow, px / 1e6),
                  "# us per call, device events around >= 0.2 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
                  "%-58s %6s %9s %9s %9s %12s" % ("variant", "reps", "median", "min", "max", "GB/s moved")]
        for name, _ in variants:
            v = res[name]
            lines.append("%-58s %6d %9.1f %9.1f %9.1f %12.1f" % (name, reps[name], med[name], min(v), max(v), moved[name] / med[name] / 1e3))
        for fmt, k in (("nv12", 0), ("p010", 1)):
            lines.append("kernel %s / copy of the same traffic = %.2f   (aim <= 2);  torch ops / kernel = %.1f"
                         % (fmt, med["kernel " + fmt] / med[variants[k][0]], med["torch ops " + fmt] / med["kernel " + fmt]))
        lines.append("")
        del variants, s, out
        torch.cuda.empty_cache()
    emit(lines[:-1])


def end_to_end():
    from bench import synth_video
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = PRESETS["R50_ovis_360"]
    model = MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()
    L, H, W = 120, 360, 640
    v = synth_video(0, L, seed=1).round().clamp(0, 255).to(torch.uint8)
    buf = torch.empty(L, H + H // 2, W, dtype=torch.uint8)          # luma: the green plane; chroma: the sub-sampled red and blue planes
    buf[:, :H] = v[:, 1]
    buf[:, H:] = torch.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(L, H // 2, W)
    surf = YuvFrames.from_surface(buf.cuda(), H, W, H)
    feeds = {"uint8 RGB tensors": yuv_to_rgb(surf), "NV12 surfaces": surf}    # the same pictures either way

    def run(feed):
        ov = model.online_video()
        t0 = time.perf_counter()
        n = 0
        for a in range(0, L, 30):
            n += len(ov.push(feed[a:a + 30]))
        n += len(ov.close())
        torch.cuda.synchronize()
        fps = L / (time.perf_counter() - t0)
        ov.result()                                # (sets model.last_num_tracks)
        return fps, n

    names = list(feeds)
    for k in names:
        run(feeds[k])
    res = {k: [] for k in names}
    for r in range(7):
        for k in (names if r % 2 == 0 else names[::-1]):
            fps, n = run(feeds[k])
            res[k].append(fps)
    lines = ["# end to end: %d frames of %d x %d, resident on the device, through online_video in pushes of 30, %d windows, tracks %d;"
             % (L, H, W, n, model.last_num_tracks),
             "# frames/s of push() .. close() with the windows on the host, 7 runs each, alternating, after one warm-up each",
             "%-20s %9s %9s %9s %12s" % ("input", "median", "min", "max", "spread %")]
    for k in names:
        x = res[k]
        lines.append("%-20s %9.1f %9.1f %9.1f %12.2f" % (k, statistics.median(x), min(x), max(x), 100 * (max(x) - min(x)) / statistics.median(x)))
    lines.append("NV12 / RGB = %.4f" % (statistics.median(res["NV12 surfaces"]) / statistics.median(res["uint8 RGB tensors"])))
    emit(lines)


if __name__ == "__main__":
    launches()
    end_to_end()
