"""Do two trees compute the same final masks on every output path?  One 17-frame synthetic video (96 x 160, output 90 x 150, windows of
6 frames so that tracks appear in later windows) through forward() with every early_masks x rle_output x geometry_output x
label_output (False, True, "only") x overlay_output x ground truth (none, seeded random masks at the output size) and through
online_video with every emit (masks, rle, labels, overlay) x geometry x keep in pushes of 1, 5 and all frames, once more with the
ground truth; everything returned is kept.

    python tools/final_mask_paths_ab.py dump OUT.pt                 # in each tree (the tool is self-contained: copy it into the other one)
    python tools/final_mask_paths_ab.py compare A.pt B.pt [--out FILE]
    python tools/final_mask_paths_ab.py bench DIR_A DIR_B [--out FILE]

`compare` prints one line per case (torch.equal on every tensor, == on everything else), `bench` one line per array that
`bench.py --dump-outputs DIR` wrote in the two trees; both exit 1 if anything differs."""
import dataclasses
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _plain(x):
    """Results as plain containers of cloned tensors (pinned views and dataclasses do not survive a save)."""
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if dataclasses.is_dataclass(x):
        return {f.name: _plain(getattr(x, f.name)) for f in dataclasses.fields(x)}
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _count(x):
    if torch.is_tensor(x):
        return 1, 0
    if isinstance(x, dict) and set(x) == {"size", "counts"}:
        return 0, 1
    vals = x.values() if isinstance(x, dict) else x if isinstance(x, list) else ()
    t = r = 0
    for v in vals:
        a, b = _count(v)
        t, r = t + a, r + b
    return t, r


def dump(path):
    from bench import synth_video
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], n_frames_window_test=6)
    model = MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()
    L, (Ho, Wo) = 17, (90, 150)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    from mdqe_cvpr2023_amd.vis_score import GroundTruth
    g = torch.Generator().manual_seed(11)
    gt = GroundTruth(masks=torch.rand(3, L, Ho // 10, Wo // 10, generator=g).gt(0.6).repeat_interleave(10, 2).repeat_interleave(10, 3),
                     category_ids=[1, 2, 3])
    out = {}
    flags = ("early_masks", "rle_output", "geometry_output", "label_output", "overlay_output")
    saved = {k: getattr(model, k) for k in flags}
    for lab, ov, scored in itertools.product((False, True, "only"), (False, True), (False, True)):
        for early, rle, geo in itertools.product((True, False), repeat=3):
            for k, v in zip(flags, (early, rle, geo, lab, ov)):
                setattr(model, k, v)
            name = "forward early=%d rle=%d geometry=%d" % (early, rle, geo)       # (the cases of before this list grew keep their names)
            if lab or ov or scored:
                name += " labels=%s overlay=%d gt=%d" % (lab, ov, scored)
            item = {"image": frames, "height": Ho, "width": Wo}
            out[name] = _plain(model([dict(item, ground_truth=gt) if scored else item]))
    for k, v in saved.items():
        setattr(model, k, v)
    for emit, geo, keep, scored in itertools.product(("masks", "rle", "labels", "overlay"), (False, True), (False, True), (False, True)):
        for name, sizes in (("1", [1] * L), ("5", [min(5, L - a) for a in range(0, L, 5)]), ("all", [L])):
            ov = model.online_video(height=Ho, width=Wo, emit=emit, keep=keep, geometry=geo, **({"ground_truth": gt} if scored else {}))
            wins, a = [], 0
            for n in sizes:
                wins += [_plain(w) for w in ov.push(frames[a:a + n])]
                a += n
            wins += [_plain(w) for w in ov.close()]
            out["online emit=%s geometry=%d keep=%d pushes=%s%s" % (emit, geo, keep, name, " gt=1" if scored else "")] = {
                "windows": wins, "result": _plain(ov.result())}
    torch.cuda.synchronize()
    torch.save(out, path)
    print("%d cases -> %s" % (len(out), path))


def compare(pa, pb):
    a, b = torch.load(pa, weights_only=False), torch.load(pb, weights_only=False)
    lines, ok = [], list(a) == list(b)
    if not ok:
        lines.append("DIFFERENT CASE LISTS: %s | %s" % (sorted(set(a) - set(b)), sorted(set(b) - set(a))))
    for k in a:
        same = k in b and _same(a[k], b[k])
        ok = ok and same
        lines.append("%-76s %3d tensors %4d RLE strings  %s" % ((k,) + _count(a[k]) + ("identical" if same else "DIFFERENT",)))
    return ok, lines


def compare_bench(da, db):
    names = sorted(f for f in os.listdir(da) if f.endswith(".npy"))
    lines, ok = [], bool(names) and names == sorted(f for f in os.listdir(db) if f.endswith(".npy"))
    for f in names if ok else ():
        x, y = np.load(os.path.join(da, f)), np.load(os.path.join(db, f))
        same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
        ok = ok and same
        lines.append("bench.py --dump-outputs %-28s %-20s %s" % (f, "x".join(map(str, x.shape)), "identical" if same else "DIFFERENT"))
    return ok, lines


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] in ("compare", "bench"):
        ok, lines = (compare if sys.argv[1] == "compare" else compare_bench)(sys.argv[2], sys.argv[3])
        lines.append("ALL IDENTICAL" if ok else "DIFFERENCES FOUND")
        print("\n".join(lines))
        if "--out" in sys.argv[4:]:
            with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
                fh.write("\n".join(lines) + "\n")
        sys.exit(0 if ok else 1)
    else:
        sys.exit(__doc__)
