"""The helpers the three batch builders share (frustum_convnet_amd/inputs.py), exercised directly on the CPU -- no kernel runs: the
packing of ragged host records, the size_class / one-hot rows, and the device refusal of every public entry method that has one."""
import re
import types

import numpy as np
import pytest
import torch

from frustum_convnet_amd import inputs

REFUSAL = "frustum_convnet_amd: input construction is a HIP kernel (MI355X only); no CPU fallback"


def test_pack_ragged_records_with_an_empty_one():
    rng = np.random.RandomState(5)
    counts = [3, 0, 5, 1]
    recs = [{"points": rng.rand(n, 4).astype(np.float64), "frustum_angle": 0.25 * i, "box2d": [i, 1, 2, 3],
             "P": np.arange(12.0).reshape(3, 4) + i} for i, n in enumerate(counts)]
    h = inputs._pack(recs, counts, (("fangle", "frustum_angle", ()), ("box2d", "box2d", (4,)), ("P", "P", (12,))))
    assert list(h) == ["raw", "off", "fangle", "box2d", "P"]
    assert h["raw"].dtype == np.float32 and h["raw"].shape == (9, 4) and h["raw"].flags.c_contiguous
    assert h["off"].dtype == np.int64 and h["off"].tolist() == [0, 3, 3, 8, 9]             # the empty record: two equal offsets
    for i in range(4):
        assert np.array_equal(h["raw"][h["off"][i]:h["off"][i + 1]], recs[i]["points"].astype(np.float32))
    assert all(h[k].dtype == np.float64 for k in ("fangle", "box2d", "P"))
    assert h["fangle"].shape == (4,) and h["fangle"].tolist() == [0.0, 0.25, 0.5, 0.75]
    assert h["box2d"].shape == (4, 4) and h["box2d"][:, 0].tolist() == [0.0, 1.0, 2.0, 3.0]
    assert h["P"].shape == (4, 12) and np.array_equal(h["P"][2], np.arange(12.0) + 2)


@pytest.mark.parametrize("one_hot", [True, False])
def test_class_rows(one_hot):
    b = types.SimpleNamespace(classes=["Car", "Pedestrian", "Cyclist"], one_hot=one_hot, device=torch.device("cpu"))
    d = {}
    inputs._class_rows(b, d, ["Cyclist", "Car", "Car", "Pedestrian"])
    assert list(d) == (["size_class", "one_hot"] if one_hot else ["size_class"])
    assert d["size_class"].dtype == torch.int64 and d["size_class"].tolist() == [[2], [0], [0], [1]]
    if one_hot:
        assert d["one_hot"].dtype == torch.float32
        assert d["one_hot"].tolist() == [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    d = {}
    inputs._class_rows(b, d, ["Pedestrian"], size_class=False)                            # the inference batches: no size_class
    assert list(d) == (["one_hot"] if one_hot else []) and (not one_hot or d["one_hot"].tolist() == [[0.0, 1.0, 0.0]])
    with pytest.raises(ValueError):
        inputs._class_rows(b, {}, ["Car", "Tram"])
    d = {}
    if one_hot:
        with pytest.raises(ValueError):
            inputs._class_rows(b, d, ["Car", "Tram"], size_class=False)
    else:                                              # nothing to write: the names are not looked up, any name passes
        inputs._class_rows(b, d, ["Car", "Tram"], size_class=False)
    assert d == {}


def test_every_public_entry_method_refuses_the_cpu():
    from frustum_convnet_amd.config import reset_cfg
    reset_cfg()
    kitti = inputs.InputBuilder(8, (0.25, 0.5, 1.0, 2.0), 70.0, device="cpu")
    sun = inputs.SunrgbdInputBuilder(8, (0.2, 0.4, 0.8, 1.6, 3.2), 8.0, device="cpu")
    refine = inputs.RefineInputBuilder(8, strides=(0.1, 0.2, 0.4, 0.8), device="cpu")
    calls = [(kitti.build, ([],)), (kitti.upload, ([],)), (kitti.build_device, ({}, None, [], [])),
             (kitti.build_device_train, ({}, None, [])), (sun.build, ([],)), (sun.build_device, ({}, None, None, [], [])),
             (sun.build_device_train, ({}, None, None, [])), (refine.build, ([],)), (refine.build_device, ({}, [])),
             (refine.build_device_train, ({}, []))]
    for fn, args in calls:
        with pytest.raises(RuntimeError, match="^" + re.escape(REFUSAL) + "$"):
            fn(*args)
