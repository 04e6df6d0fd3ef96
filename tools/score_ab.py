"""A/B of scoring a video against ground truth on the device (mdqe_final_masks_overlap, vis_score.py).

  score_ab.py kernel OUT [H W FRAMES]   the overlap kernel alone, G = 8 and G = 32 ground-truth tracks, against the label-map kernel
                                        (mdqe_final_label_map_u8, with and without geometry: the same per-pixel work, the yardstick)
                                        and the dense kernel with geometry, on one window of 15 tracks: the shipped 360p one (30 frames
                                        of 360 x 640) or one of FRAMES frames of H x W -- the label map's own A/B shapes.
  score_ab.py e2e OUT [FRAMES]          the bench's 360p video (pinned host frames, workload initialisation) through model(): without
                                        ground truth, with it (packed words resident on the device / a ground truth's first use, its
                                        words uploaded from the host inside the call), with it and label_output = "only" (no dense plane
                                        at all), and the alternative a user has without this kernel: the plain run plus numpy video IoU
                                        on the dense masks it brought to the host.  The variants alternate in ONE process (a comparison
                                        needs that); an error in any of them ends the process at once.
  score_ab.py all OUT                   what profiles/score_overlap_ab.txt holds: the 360p kernel table, the 640 x 1138 one and the
                                        end-to-end one, each as a child process of its own under its own time limit (150, 150 and 240 s);
                                        a child that fails or runs out of time ends the run, nothing more is started after it.
The table is appended to OUT.  One mode per process."""
import os, sys, statistics, time
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import ops

mode, out_path = sys.argv[1], sys.argv[2]

if mode == "all":
    import subprocess
    for args, limit in ((["kernel", out_path], 150), (["kernel", out_path, "640", "1138", "30"], 150), (["e2e", out_path], 240)):
        try:
            status = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=limit).returncode
        except subprocess.TimeoutExpired:                 # (run() has killed the child)
            status = 124
        if status != 0:
            raise SystemExit("score_ab.py %s ended with status %d: nothing more is started" % (" ".join(args), status))
    raise SystemExit(0)


def emit(lines):
    with open(out_path, "a") as fh:
        fh.write("\n".join(lines) + "\n\n")
    print("\n".join(lines))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps     # us per call


if mode == "kernel":
    h, w, Fw = (int(v) for v in sys.argv[3:6]) if len(sys.argv) > 5 else (360, 640, 30)
    n, Hm, Wm, Ho, Wo = 15, (h + 31) // 32 * 8, (w + 31) // 32 * 8, h, w
    g = torch.Generator().manual_seed(0)
    lg = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    # ground truth: 32 blob tracks of the same kind as the predictions', at the output size; G = 8 uses the first 8 bits of the words
    words = torch.zeros(Fw, Ho, Wo, dtype=torch.int32, device="cuda")
    planes = []
    for b in range(32):
        p = (F.interpolate(torch.randn(1, Fw, 12, 20, generator=g) * 3, size=(Ho, Wo), mode="bilinear")[0] - 1.0 > 0).cuda()
        planes.append(p)
        words |= p.to(torch.int32) * (1 << b if b < 31 else -2 ** 31)
    words8 = (words & 0xFF).view(torch.uint32)
    words = words.view(torch.uint32)
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    out = torch.empty(n, Fw, Ho, Wo, dtype=torch.uint8, device="cuda")
    lab = torch.empty(Fw, Ho, Wo, dtype=torch.uint8, device="cuda")
    geom = torch.empty(n * Fw, 5, dtype=torch.int32, device="cuda")
    inter = torch.zeros(n, 32, dtype=torch.int64, device="cuda")
    area = torch.empty(n * Fw, dtype=torch.int32, device="cuda")
    os.environ.pop("MDQE_LABEL_MAP_STAGE", None)

    def u8_geom(): ops.final_masks_geom(lg, idx, 4, h, w, Ho, Wo, out, 0, geom=geom)
    def label(): ops.final_label_map(lg, idx, 4, h, w, Ho, Wo, lab, 0)
    def label_geom(): ops.final_label_map(lg, idx, 4, h, w, Ho, Wo, lab, 0, geom=geom)
    def overlap8(): ops.final_masks_overlap(lg, idx, 4, h, w, Ho, Wo, words8, 8, 0, inter, area)
    def overlap32(): ops.final_masks_overlap(lg, idx, 4, h, w, Ho, Wo, words, 32, 0, inter, area)

    variants = [("mdqe_final_masks_u8_geom", u8_geom), ("mdqe_final_label_map_u8", label), ("mdqe_final_label_map_u8 + geom", label_geom),
                ("mdqe_final_masks_overlap G = 8", overlap8), ("mdqe_final_masks_overlap G = 32", overlap32)]
    # sanity: the counts are torch's on the dense masks
    u8_geom()
    masks = out.view(torch.bool)
    overlap32()
    torch.cuda.synchronize()
    want = torch.stack([torch.stack([(masks[k] & planes[b]).sum() for b in range(32)]) for k in range(n)])
    assert torch.equal(inter, want) and torch.equal(area.view(n, Fw).long(), masks.flatten(2).sum(2))
    inter.zero_(); overlap8(); torch.cuda.synchronize()
    assert torch.equal(inter[:, :8], want[:, :8]) and not bool(inter[:, 8:].any())
    reps = {}
    for name, fn in variants:
        for _ in range(5): fn()
        torch.cuda.synchronize()
        reps[name] = max(20, int(0.25e6 / timed(fn, 20)) + 1)
    res = {name: [] for name, _ in variants}
    for r in range(7):
        for name, fn in variants:
            res[name].append(timed(fn, reps[name]))
    med = {name: statistics.median(v) for name, v in res.items()}
    empty_pairs = float((want == 0).float().mean())
    lines = ["# one tracker window: n = %d tracks x %d frames, Hm x Wm = %d x %d, h, w = Ho, Wo = %d, %d; logits read %.1f MB, ground-truth words read %.1f MB"
             % (n, Fw, Hm, Wm, Ho, Wo, lg.numel() * 4 / 1e6, words.numel() * 4 / 1e6),
             "# read back: overlap %d + %d integers; label map %.1f MB; dense planes %.1f MB" % (n * 32, n * Fw, Fw * Ho * Wo / 1e6, n * Fw * Ho * Wo / 1e6),
             "# us per call (the overlap entry point = its area memset + its kernel), device events around >= 0.25 s of back-to-back calls, 7 alternations in one process",
             "# (track, ground-truth track) pairs without a common pixel: %.1f %%" % (100.0 * empty_pairs),
             "%-40s %6s %9s %9s %9s" % ("variant", "reps", "median", "min", "max")]
    for name, _ in variants:
        v = res[name]
        lines.append("%-40s %6d %9.1f %9.1f %9.1f" % (name, reps[name], med[name], min(v), max(v)))
    for G in (8, 32):
        lines.append("overlap G = %-2d / label map          = %.3f   (/ label map + geom: %.3f)" % (
            G, med["mdqe_final_masks_overlap G = %d" % G] / med["mdqe_final_label_map_u8"],
            med["mdqe_final_masks_overlap G = %d" % G] / med["mdqe_final_label_map_u8 + geom"]))
    emit(lines)

elif mode == "e2e":
    import bench
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    from mdqe_cvpr2023_amd.vis_score import GroundTruth, iou_table
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 120
    cfg = PRESETS["R50_ovis_360"]
    fh, fw = bench.FRAME_SIZES["R50_ovis_360"]
    sd = random_state(cfg, seed=0, remove_zero_init_trap=True)
    model = MDQE(cfg, state_dict=sd).eval()
    bench.calibrate_synthetic_scores(model, sd, cfg, fh, fw)
    video = bench.synth_video(0, L, seed=0, h=fh, w=fw).pin_memory()
    frames = list(video)
    inp = {"image": frames, "height": fh, "width": fw}
    res0 = model([inp])
    pm = torch.stack(res0["pred_masks"])
    gm = torch.stack([torch.roll(pm[j], (3 + j % 4, 5 + j % 7), dims=(1, 2)) for j in range(pm.shape[0])])
    cats = list(res0["pred_labels"])
    gt_dev = GroundTruth(masks=gm.cuda(), category_ids=cats)                 # packed words resident on the device
    gt_host = GroundTruth(masks=gm, category_ids=cats)                       # packed words on the host: a first use uploads them inside the call
    gm_np = gm.numpy()

    def plain(): return model([inp])
    def scored_dev(): return model([dict(inp, ground_truth=gt_dev)])

    def scored_host():
        gt_host._on.clear()                                                  # (GroundTruth.on keeps the device copy: forget it, every call is a first use)
        return model([dict(inp, ground_truth=gt_host)])

    def scored_only():
        model.label_output = "only"
        try:
            return model([dict(inp, ground_truth=gt_dev)])
        finally:
            model.label_output = False

    def plain_numpy():
        r = model([inp])
        p = [m.numpy() for m in r["pred_masks"]]
        inter = np.array([[np.count_nonzero(a & b) for b in gm_np] for a in p], dtype=np.int64)
        pa = np.array([[np.count_nonzero(f) for f in a] for a in p], dtype=np.int64)
        r["iou"] = iou_table(inter, pa, gt_host.gt_area.numpy())
        return r

    variants = [("model(), no ground truth", plain), ("model(), ground truth on the device", scored_dev),
                ("model(), ground truth's first use (words uploaded)", scored_host), ("model(), ground truth, label_output = 'only'", scored_only),
                ("model() + numpy IoU on the host's dense masks", plain_numpy)]
    ref = scored_dev()["pred_gt"]
    assert np.array_equal(plain_numpy()["iou"], ref["iou"].numpy())         # the two ways agree to the bit
    assert torch.equal(scored_only()["pred_gt"]["inter"], ref["inter"]) and torch.equal(scored_host()["pred_gt"]["inter"], ref["inter"])
    res = {name: [] for name, _ in variants}
    for r in range(5):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: statistics.median(v) for name, v in res.items()}
    base = med["model(), no ground truth"]
    lines = ["# the bench's 360p video: %d frames of %d x %d from pinned host memory, R50_ovis_360, workload initialisation, fp32" % (L, fh, fw),
             "# %d outputs over %d tracks against %d ground-truth tracks (the run's own masks rolled by a few pixels); mean IoU of the diagonal %.3f"
             % (len(res0["pred_scores"]), model.last_num_tracks, gt_dev.G, float(np.diag(ref["iou"].numpy()).mean())),
             "# ms per video, host clock around the call and a device synchronise, 5 alternations of all variants in one process after one warm-up of each",
             "%-52s %9s %9s %9s %9s" % ("variant", "median", "min", "max", "- plain")]
    for name, _ in variants:
        v = res[name]
        lines.append("%-52s %9.1f %9.1f %9.1f %+9.1f" % (name, med[name], min(v), max(v), med[name] - base))
    emit(lines)
else:
    raise SystemExit("score_ab.py kernel|e2e OUT ...")
