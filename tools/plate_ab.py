"""What object removal costs: one tracker window's label + overlay stage (ops.final_label_map, ops.final_matte, then
ops.render_replace) with replace="tracks" on a colour -- the stage as it was -- against backdrop="plate": between the matte and the
painter the plate's margin (one ops.grow_labels launch, none at margin 0), one ops.plate_update over the window's 30 frames and one
ops.plate_picture, as merge.Plate does it, at margin 0 / 4 / 16 (reach 16) and reach 0 / 16 / 32 (margin 4); the same on NV12
surfaces; on the two windows of tools/grow_ab.py: 15 tracks x 30 frames of 360 x 640 of the bench's synthetic video, DENSE (nearly every
pixel belongs to a track: little is ever seen, every tile of the picture is searched) and SPARSE (small tracks: most pixels teach the
plate, most tiles skip the search).  The plate's state stays warm over the repetitions, as it does over a video's windows.  Then,
`plate_ab.py OUT e2e`, frames/s of a warm 120-frame 360p online_video(emit="overlay") session with Style(), with replace="tracks" on a
colour and, where the style has the field, with the plate (run the first two on the parent commit too: the untouched paths).  One
process, no retries.  Tables are appended to OUT when given."""
import os, sys, statistics, time
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdqe_cvpr2023_amd import merge, ops
from mdqe_cvpr2023_amd.preprocess import YuvFrames
from mdqe_cvpr2023_amd.render import Style

HAS_PLATE = "plate_frames" in Style.__dataclass_fields__        # (the parent commit runs the baselines only)
KNOBS = ((0, 16), (4, 16), (16, 16), (4, 0), (4, 32))           # (plate_margin, plate_reach)


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
    Hm, Wm = (h + 31) // 32 * 8, (w + 31) // 32 * 8                          # (the workload of tools/grow_ab.py)
    g = torch.Generator().manual_seed(0)
    dense = (F.interpolate(torch.randn(n, Fw, 12, 20, generator=g) * 3, size=(Hm, Wm), mode="bilinear") - 1.0).contiguous().cuda()
    sparse = (dense - 7.0).contiguous()                                      # the same blobs, only their peaks: small tracks
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    lab = torch.empty(Fw, h, w, dtype=torch.uint8, device="cuda")
    mat = torch.empty_like(lab)
    v = synth_video(0, Fw, seed=1).round().clamp(0, 255).to(torch.uint8)
    fr8 = v.cuda()
    out = torch.empty(Fw, h, w, 3, dtype=torch.uint8, device="cuda")
    s = YuvFrames.empty(Fw, h, w, device="cuda")                             # luma from the green plane, chroma from sub-sampled red and blue
    s.y.copy_(v[:, 1])
    s.uv.copy_(torch.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(Fw, h // 2, w))
    so = YuvFrames.empty(Fw, h, w, device="cuda")

    def stage(st, lg, surface=False):
        pal = st.palette_yuv_on("cuda", *s.meta()[2:]) if surface else st.palette_on("cuda")
        act, take = st.actions_on("cuda"), st.takes_on("cuda")
        plate = merge.Plate(st, (h, w), torch.device("cuda"), s.meta() if surface else None) if HAS_PLATE and st.plate else None
        back = None if plate is not None else st.backdrop_yuv_on("cuda", *s.meta()[2:]) if surface else st.backdrop_on("cuda")

        def run():
            ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
            ops.final_matte(lg, idx, 4, h, w, h, w, mat, 0, take, st.matte_gain)
            b = back
            if plate is not None:
                plate.observe(lab, 0, Fw, [(s if surface else fr8, 0)])
                b = plate.picture()
            if surface: ops.render_replace_yuv(lab, s, pal, act, mat, b, so, 0, st.a256, st.contour, "tracks")
            else: ops.render_replace(lab, fr8, pal, act, mat, b, out, 0, st.a256, st.contour, "tracks")
        return run
    groups = (("", dense, False), ("sparse: ", sparse, False), ("NV12: ", dense, True))
    variants = []
    for tag, lg, surface in groups:
        variants.append((tag + "label + matte + replace='tracks' on a colour (as it was)", stage(Style(replace="tracks"), lg, surface)))
        if HAS_PLATE:
            variants += [(tag + "... backdrop='plate', margin %d, reach %d" % (m, r),
                          stage(Style(replace="tracks", backdrop="plate", plate_margin=m, plate_reach=r), lg, surface)) for m, r in KNOBS]
    per = len(variants) // len(groups)
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

    def share(lg):                                                            # pixels of a track, and pixels no frame of the window sees free
        ops.final_label_map(lg, idx, 4, h, w, h, w, lab, 0)
        return float((lab != 0).float().mean()), float((lab != 0).all(0).float().mean())
    (pd, nd), (ps, ns) = share(dense), share(sparse)
    lines = ["# one tracker window: n = %d tracks x %d frames of %d x %d (bench.synth_video, uint8)" % (n, Fw, h, w),
             "# dense window: %.1f %% of the pixels belong to a track, %.1f %% are covered in every frame; sparse window: %.2f %% and %.2f %%"
             % (100 * pd, 100 * nd, 100 * ps, 100 * ns),
             "# us per call, device events around >= 0.25 s of back-to-back calls, 7 passes over all variants in one process, order alternating",
             "# '- colour' and '/ colour': against the first line of the variant's own group",
             "%-72s %6s %9s %9s %9s %9s %8s" % ("variant", "reps", "median", "min", "max", "- colour", "/ colour")]
    for i, (name, _) in enumerate(variants):
        x = res[name]
        base = med[variants[i - i % per][0]]
        lines.append("%-72s %6d %9.1f %9.1f %9.1f %9.1f %8.2f" % (name, reps[name], med[name], min(x), max(x), med[name] - base, med[name] / base))
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
    kinds = {"Style()": Style(), "Style(replace='tracks')": Style(replace="tracks")}
    if HAS_PLATE:
        kinds["Style(replace='tracks', backdrop='plate')"] = Style(replace="tracks", backdrop="plate")
        kinds["... plate_margin=0"] = Style(replace="tracks", backdrop="plate", plate_margin=0)
        kinds["... plate_margin=16, plate_reach=32"] = Style(replace="tracks", backdrop="plate", plate_margin=16, plate_reach=32)

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
