"""Per-frame track label maps, the host side: the three rle.py helpers on hand-made maps, the errors that need no launch (a config whose
tracker bank does not fit uint8 labels, a bad `emit`, the wrapper's argument checks) and the ABI entry."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _map():
    """[2, 4, 5]: tracks 0, 2 and 6 (labels 1, 3, 7) and background."""
    lm = np.zeros((2, 4, 5), dtype=np.uint8)
    lm[0, :2, :3] = 1
    lm[0, 2:, 3:] = 3
    lm[1, 1:3, 1:4] = 7
    lm[1, 0, 0] = 1
    return lm


@pytest.mark.parametrize("as_tensor", [False, True])
def test_labels_to_masks_and_keep(as_tensor):
    from mdqe_cvpr2023_amd import rle as R
    lm = _map()
    x = torch.from_numpy(lm) if as_tensor else lm
    m = R.labels_to_masks(x, [2, 0, 5, 6])
    assert isinstance(m, torch.Tensor if as_tensor else np.ndarray)
    m = np.asarray(m)
    assert m.dtype == np.bool_ and m.shape == (4, 2, 4, 5)
    assert np.array_equal(m[0], lm == 3) and np.array_equal(m[1], lm == 1) and not m[2].any() and np.array_equal(m[3], lm == 7)
    assert np.array_equal(m.any(0), lm != 0) and int(m.sum()) == int((lm != 0).sum())          # exclusive: no pixel twice
    assert R.labels_to_masks(x, []).shape == (0, 2, 4, 5)
    k = R.labels_keep(x, [0, 6])
    assert isinstance(k, torch.Tensor if as_tensor else np.ndarray)
    k = np.asarray(k)
    assert k.dtype == np.uint8 and k.shape == lm.shape
    assert np.array_equal(k, np.where(lm == 3, 0, lm)) and np.array_equal(np.asarray(R.labels_keep(x, [])), np.zeros_like(lm))
    assert np.array_equal(np.asarray(R.labels_keep(x, [0, 2, 6, 254])), lm)
    for bad in (-1, 255):
        with pytest.raises(ValueError):
            R.labels_keep(x, [bad])


def test_labels_to_rles():
    import rle_oracle as RO
    from mdqe_cvpr2023_amd import rle as R
    lm = _map()
    for x in (lm, torch.from_numpy(lm)):
        for t in (0, 2, 6, 9):
            rles = R.labels_to_rles(x, t)
            assert len(rles) == 2
            for f, r in enumerate(rles):
                assert r["size"] == [4, 5] and r["counts"].encode() == RO.encode(lm[f] == t + 1)["counts"]
                assert np.array_equal(RO.rle_decode(RO.rle_from_string(r["counts"].encode()), 4, 5), lm[f] == t + 1)
    assert R.labels_to_rles(lm, 9)[0] == R.empty_rle((4, 5))


def _cpu_model(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    return MDQE(dataclasses.replace(PRESETS["R50_ovis_360"], **kw), seed=1)


def test_label_output_values_and_the_uint8_limit():
    big, ok = _cpu_model(n_max_inst=256), _cpu_model(n_max_inst=255)
    assert big.label_output is False and ok.label_output is False
    for v in (True, "only"):
        with pytest.raises(ValueError, match="n_max_inst"):
            big.label_output = v
        assert big.label_output is False
        ok.label_output = v
        assert ok.label_output == v
    big.label_output = False                                          # switching it off is always allowed
    ok.label_output = False
    for bad in ("labels", 1.5, None):
        with pytest.raises(ValueError, match="label_output"):
            ok.label_output = bad
    assert ok.label_output is False
    # online sessions: the emit check comes first, then the same limit; neither needs a device
    with pytest.raises(ValueError, match="emit"):
        ok.online_video(emit="label")
    with pytest.raises(ValueError, match="n_max_inst"):
        big.online_video(emit="labels")


def test_wrapper_argument_checks_come_before_any_launch():
    from mdqe_cvpr2023_amd import ops
    lg = torch.zeros(3, 2, 4, 6)
    idx = torch.arange(3, dtype=torch.int32)
    out = torch.zeros(4, 16, 24, dtype=torch.uint8)
    call = lambda lg=lg, idx=idx, out=out, f_off=0: ops.final_label_map(lg, idx, 4, 16, 24, 16, 24, out, f_off)
    with pytest.raises(RuntimeError, match="n <= 255"):
        call(lg=torch.zeros(256, 1, 4, 6))
    with pytest.raises(RuntimeError, match="inst_idx must be int32"):
        call(idx=idx.long())
    for bad in (out.float(), out[:, :, :20], out[:1], out.view(4, 1, 16, 24), torch.zeros(4, 16, 48, dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(RuntimeError, match="out must be contiguous CUDA uint8"):
            call(out=bad)
    with pytest.raises(RuntimeError, match="out must be contiguous CUDA uint8"):
        call(f_off=3)                                                 # 3 + Fw > 4 frames
    with pytest.raises(RuntimeError, match="out must be contiguous CUDA uint8"):
        call(f_off=-1)
    with pytest.raises(RuntimeError, match="out must be contiguous CUDA uint8"):
        call()                                                        # right shape and dtype, but a host tensor


def test_abi_declares_exports_and_binds_the_label_map_entry_point():
    from mdqe_cvpr2023_amd import _lib
    name = "mdqe_final_label_map_u8"
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
    assert hasattr(h, name) and name in _lib.SIGNATURES
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == 15
    assert h.mdqe_abi_version() == 6                                  # no existing entry changed
    # n_sel > 255 is refused by the entry point itself, before any pointer is looked at (no launch)
    assert h.mdqe_final_label_map_u8(None, 256, None, 1, 4, 6, 4, 16, 24, 16, 24, None, 0, None, None) != 0


def test_window_has_labels_and_its_fields_are_what_they_were():
    from mdqe_cvpr2023_amd import online
    assert [f.name for f in dataclasses.fields(online.Window)] == ["frames", "track_ids", "cls_probs", "masks", "rles", "boxes", "areas"]
    w = online.Window(frames=(0, 1), track_ids=[], cls_probs=torch.zeros(0, 2))
    assert w.labels is None and w.masks is None
    lab = torch.zeros(1, 2, 3, dtype=torch.uint8)
    assert online.Window(frames=(0, 1), track_ids=[], cls_probs=torch.zeros(0, 2), labels=lab).labels is lab
