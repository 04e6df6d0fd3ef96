"""Online video inference (MDQE.online_video) against forward() on the bench's R50 360p workload: 120 synthetic frames in pinned host
memory, the bench's calibrated synthetic weights.  Runs alternate -- forward(), then online at each push size -- and every figure is
the median of REPS runs:
  * frames/s of the whole video (first push .. result());
  * per-window latency: duration of the push() (or close()) call that returned the window, i.e. from the call that completes
    the window's flush clip to the window's masks on the host -- median and worst over all windows of all runs;
  * peak device memory above the model's resident state (torch.cuda.max_memory_allocated; frames in pinned host memory).

    python tools/online_throughput.py [REPS] [OUT]           -> profiles/r08_online_push_sizes.txt
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FRAME_SIZES, calibrate_synthetic_scores, synth_video  # noqa: E402
from mdqe_cvpr2023_amd.config import PRESETS  # noqa: E402
from mdqe_cvpr2023_amd.meta_arch import MDQE  # noqa: E402
from mdqe_cvpr2023_amd.params import random_state  # noqa: E402

PUSH_SIZES = (1, 4, 10, 30, 120)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out = sys.argv[2] if len(sys.argv) > 2 else None
    cfg = PRESETS["R50_ovis_360"]
    fh, fw = FRAME_SIZES["R50_ovis_360"]
    sd = random_state(cfg, seed=0, remove_zero_init_trap=True)
    model = MDQE(cfg, state_dict=sd).eval()
    calibrate_synthetic_scores(model, sd, cfg, fh, fw)
    L = 120
    video = synth_video(0, L, seed=0, h=fh, w=fw).pin_memory()
    host_frames = list(video)

    def offline():
        t0 = time.perf_counter()
        r = model([{"image": host_frames, "height": fh, "width": fw}])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, [], r

    def online(ps):
        lat = []
        t0 = time.perf_counter()
        ov = model.online_video()
        for a in range(0, L, ps):
            t1 = time.perf_counter()
            ws = ov.push(video[a:a + ps])
            lat += [time.perf_counter() - t1] * len(ws)
        t1 = time.perf_counter()
        ws = ov.close()
        lat += [time.perf_counter() - t1] * len(ws)
        r = ov.result()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, lat, r

    legs = [("forward()", offline)] + [("push %d" % ps, (lambda ps=ps: lambda: online(ps))()) for ps in PUSH_SIZES]
    for _, fn in legs:                                   # warm-up: kernels, streams, allocator blocks, pinned pools
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    stats = {name: {"t": [], "lat": [], "peak": []} for name, _ in legs}
    for _ in range(reps):
        for name, fn in legs:
            torch.cuda.reset_peak_memory_stats()
            t, lat, r = fn()
            stats[name]["t"].append(t)
            stats[name]["lat"] += lat
            stats[name]["peak"].append(torch.cuda.max_memory_allocated() - base)
            del r
    lines = ["# online video inference vs forward(): R50_ovis_360 preset, %dx%d, %d synthetic frames in pinned host memory (bench.py's "
             "workload and weights), T=%d stride=%d window=%d" % (fh, fw, L, cfg.n_frames_test, cfg.clip_stride, cfg.n_frames_window_test),
             "# median of %d alternating runs per row; window latency = the push()/close() call that returned the window "
             "(median / max over all windows of all runs); peak = max_memory_allocated above the model's resident state" % reps,
             "%-10s %10s %8s %14s %14s %12s" % ("run", "frames/s", "vs fwd", "win lat med", "win lat max", "peak MB")]
    f_ref = L / statistics.median(stats["forward()"]["t"])
    for name, _ in legs:
        s = stats[name]
        fps = L / statistics.median(s["t"])
        lm = "%.1f ms" % (1e3 * statistics.median(s["lat"])) if s["lat"] else "-"
        lx = "%.1f ms" % (1e3 * max(s["lat"])) if s["lat"] else "-"
        lines.append("%-10s %10.1f %7.1f%% %14s %14s %12.0f" % (name, fps, 100.0 * (fps / f_ref - 1), lm, lx,
                                                                statistics.median(s["peak"]) / 2 ** 20))
    txt = "\n".join(lines) + "\n"
    print(txt, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
