"""What the occlusion table costs: one tracker window's label stage (ops.final_label_map) alone, the occlusion sweep
(ops.final_occlusion) alone, the two together, and beside them the matte sweep (ops.final_matte) as the yardstick for one more pass over
the logits.  The workload of tools/trails_ab.py: one window of 15 tracks x 30 frames of 360 x 640, the dense label generator of
tools/overlay_ab.py (most pixels carry several bits: every lane walks the overlap path), the sparse window of tools/blur_ab.py (the same
blobs, only their peaks) and, as the worst case of the counting path, the dense window lifted until every pixel carries all 15 bits.
Beside it the host alternative a caller has today: the dense planes and the label map read back into pinned memory, then the counts in
numpy (held to the kernel's integers here).  `OUT e2e`: a warm 120-frame online_video(emit="rle") session with and without the option
(run the leg without it on the parent commit too: the untouched path).  Tables are appended to OUT when given."""
import os, sys, statistics, time
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops


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


def host_table(planes, labels, n):
    """The rule of include/mdqe_hip.h on the host from what was read back: per (track, frame) one bincount of the labels under the plane."""
    Fw = labels.shape[0]
    occ = np.zeros((n, Fw, n), dtype=np.int32)
    for k in range(n):
        for f in range(Fw):
            occ[k, f] = np.bincount(labels[f][planes[k, f] != 0], minlength=256)[1:n + 1]
    return occ


def launches():
    h, w, Fw, n = 360, 640, 30, 15
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/overlay_ab.py)
    g = torch.Generator().manual_seed(0)
    dense = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    sparse = (dense - 7.0).contiguous()                                      # the same blobs, only their peaks: small tracks
    every = (dense + 20.0).contiguous()                                      # every pixel carries all n bits
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    mat = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    planes = torch.empty(n, Fw, h, w, dtype=torch.uint8, device="cuda")
    occ = torch.empty(n, Fw, n, dtype=torch.int32, device="cuda")

    def label(lg): return lambda: ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
    def sweep(lg): return lambda: ops.final_occlusion(lg, idx, 4, h, w, h, w, occ)
    def matte(lg): return lambda: ops.final_matte(lg, idx, 4, h, w, h, w, mat, 0)
    def both(lg):
        a, b = label(lg), sweep(lg)
        def run():
            a(); b()
        return run
    variants = []
    for tag, lg in (("dense", dense), ("sparse", sparse), ("all bits", every)):
        variants += [("%s: label stage alone (ops.final_label_map)" % tag, label(lg)),
                     ("%s: occlusion sweep alone (ops.final_occlusion)" % tag, sweep(lg)),
                     ("%s: label stage + occlusion sweep" % tag, both(lg)),
                     ("%s: matte sweep alone (ops.final_matte)" % tag, matte(lg))]
    pin = {"planes": torch.empty(planes.shape, dtype=torch.uint8, pin_memory=True), "lab": torch.empty(lab.shape, dtype=torch.uint8, pin_memory=True)}

    def read_back():
        ops.final_masks(dense, idx, 4, h, w, h, w, planes, 0)
        label(dense)()
        pin["planes"].copy_(planes, non_blocking=True)
        pin["lab"].copy_(lab, non_blocking=True)
    variants.append(("dense: planes + label stage + read-back of both", read_back))
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
    # what the windows hold, and the host's numpy pass on what was read back, held to the kernel's integers
    stats = []
    for lg in (dense, sparse, every):
        t = ops.final_occlusion(lg, idx, 4, h, w, h, w).cpu().numpy().astype(np.int64)
        area, vis = t.sum(-1), t[np.arange(n), :, np.arange(n)]
        stats.append((float(area.sum()) / (Fw * h * w), float((area - vis).sum()) / max(float(area.sum()), 1.0)))
    read_back()
    sweep(dense)()
    torch.cuda.synchronize()
    host_t = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = host_table(pin["planes"].numpy(), pin["lab"].numpy(), n)
        host_t.append((time.perf_counter() - t0) * 1e6)
    same = np.array_equal(got, occ.cpu().numpy())
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d" % (n, Fw, h, w),
             "# set bits per pixel (the masks' areas over the frame) and the share of them that another track owns: dense %.2f and %.1f %%, "
             "sparse %.4f and %.1f %%, all bits %.2f and %.1f %%" % (stats[0][0], 100 * stats[0][1], stats[1][0], 100 * stats[1][1], stats[2][0], 100 * stats[2][1]),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "%-58s %6s %9s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "- label", "/ label")]
    for name, _ in variants:
        x, b = res[name], med[name.split(":")[0] + ": label stage alone (ops.final_label_map)"]
        lines.append("%-58s %6d %9.1f %9.1f %9.1f %9.1f %8.2f" % (name, reps[name], med[name], min(x), max(x), med[name] - b, med[name] / b))
    base = med[variants[0][0]]
    lines.append("host alternative: the planes and the map read back (%.1f us beyond the label stage) + numpy counts on the host: %.0f us (min of 3; "
                 "one bincount per track and frame); integers equal to the kernel's: %s" % (med[variants[-1][0]] - base, min(host_t), same))
    lines.append("so on the dense window the sweep costs %.2fx the label stage and %.2fx the matte sweep; the host route costs %.0fx the sweep"
                 % (med[variants[1][0]] / base, med[variants[1][0]] / med[variants[3][0]], (med[variants[-1][0]] + min(host_t)) / med[variants[1][0]]))
    emit(lines)


def end_to_end():
    from bench import synth_video
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.merge import Forms
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = PRESETS["R50_ovis_360"]
    model = MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()
    L, h, w = 120, 360, 640
    feed = synth_video(0, L, seed=1).round().clamp(0, 255).to(torch.uint8).cuda()
    kinds = {"emit='rle'": {}}
    if "occlusion" in Forms.__dataclass_fields__:   # (the parent commit runs the first leg only)
        kinds["emit='rle', occlusion=True"] = {"occlusion": True}

    def run(kind):
        ov = model.online_video(emit="rle", **kinds[kind])
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
    lines = ["# end to end: %d frames of %d x %d (resident on the device) through online_video(emit='rle') in pushes of 30, %d windows, tracks %d;"
             % (L, h, w, n, model.last_num_tracks),
             "# frames/s of push() .. close() with the windows on the host, 7 runs each in one process, order alternating, after one warm-up each",
             "%-44s %9s %9s %9s %12s" % ("session", "median", "min", "max", "/ emit='rle'")]
    for key in order:
        x = res[key]
        lines.append("%-44s %9.1f %9.1f %9.1f %12.3f" % (key, statistics.median(x), min(x), max(x),
                                                         statistics.median(x) / statistics.median(res["emit='rle'"])))
    emit(lines)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "e2e":
        end_to_end()
    else:
        launches()
