"""The visibility de-duplication's C ABI and Python surface without a GPU: the symbol, the
structs, and the rejections that happen before any device work."""
import ctypes

import pytest

FAKE = 0x1000   # never dereferenced: validation fails first
INVALID = 1


def _err():
    from aarmvs import lib
    return lib().aarmvs_last_error().decode()


def _cams(nsrc):
    from aarmvs import _lib
    return (ctypes.c_float * _lib.fusion_cam_floats(nsrc))()


def _args(cams, nsrc=2):
    from aarmvs import _lib
    a = _lib.FusionArgs()
    a.H, a.W, a.nsrc = 8, 8, nsrc
    a.ref_depth, a.confidence = FAKE, FAKE + 0x100
    for v in range(nsrc):
        a.src_depth[v] = FAKE + 0x200 + 0x100 * v
    a.cams = ctypes.addressof(cams)
    a.photo_threshold = 0.35
    a.photo_mask, a.geo_mask, a.final_mask, a.depth_avg = 0x3000, 0x3100, 0x3200, 0x3300
    return a


def _dedup(nsrc=2):
    from aarmvs import _lib
    d = _lib.FusionDedupArgs()
    d.used_ref = 0x4000
    for v in range(nsrc):
        d.used_src[v] = 0x4100 + 0x100 * v
    d.emit_mask = 0x5000
    return d


def _call(a, d):
    from aarmvs import lib
    return lib().aarmvs_fusion_filter_dedup(ctypes.byref(a), None if d is None else ctypes.byref(d), None)


def test_symbol_and_structs():
    from aarmvs import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "aarmvs_fusion_filter_dedup") and "aarmvs_fusion_filter_dedup" in _lib.SIGNATURES
    assert [f[0] for f in _lib.FusionDedupArgs._fields_] == ["used_ref", "used_src", "emit_mask"]
    assert ctypes.sizeof(_lib.FusionDedupArgs) == (2 + _lib.MAX_FUSION_SRC) * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.MAX_FUSION_SRC == 10


def test_the_plain_filter_struct_did_not_change():
    from aarmvs import _lib
    assert [f[0] for f in _lib.FusionArgs._fields_] == [
        "H", "W", "nsrc", "ref_depth", "confidence", "src_depth", "cams", "photo_threshold", "photo_mask",
        "geo_mask", "final_mask", "depth_avg"]
    p = ctypes.sizeof(ctypes.c_void_p)
    # 3 ints (+ padding), 2 + 10 + 1 pointers, a float (+ padding), 4 pointers
    assert ctypes.sizeof(_lib.FusionArgs) == 16 + 13 * p + 8 + 4 * p == 160
    assert _lib.FusionArgs.depth_avg.offset == 152


def test_the_profiler_list_did_not_change():
    """The de-duplicating launch is timed under the plain filter's id, "fusion": the list of names
    is pinned by the earlier ABI tests (its last entry and its length)."""
    from aarmvs import lib
    L = lib()
    names = [L.aarmvs_profile_kernel_name(i).decode() for i in range(L.aarmvs_profile_kernel_count())]
    assert names.index("fusion") == 2 and names[-1] == "refine" and len(names) == 58
    assert len(set(names)) == len(names)


def test_rejects_a_null_emit_mask():
    cams = _cams(2)
    a, d = _args(cams), _dedup()
    d.emit_mask = None
    assert _call(a, d) == INVALID
    assert "fusion_filter_dedup" in _err() and "emit_mask" in _err()


@pytest.mark.parametrize("v", [0, 1])
def test_rejects_a_reference_view_that_is_its_own_source(v):
    cams = _cams(2)
    a, d = _args(cams), _dedup()
    d.used_src[v] = d.used_ref
    assert _call(a, d) == INVALID
    assert "fusion_filter_dedup" in _err() and "used_ref" in _err() and "used_src" in _err()


@pytest.mark.parametrize("mask", ["photo_mask", "geo_mask", "final_mask"])
def test_rejects_an_emit_mask_that_is_another_mask(mask):
    cams = _cams(2)
    a, d = _args(cams), _dedup()
    d.emit_mask = getattr(a, mask)
    assert _call(a, d) == INVALID
    assert "fusion_filter_dedup" in _err() and "emit_mask" in _err()


def test_the_plain_filters_validation_still_applies():
    from aarmvs import lib
    cams = _cams(2)
    a, d = _args(cams), _dedup()
    a.nsrc = 11
    assert _call(a, d) == INVALID and _err() == "fusion_filter: need H, W >= 1 and 1 <= nsrc <= 10"
    a = _args(cams)
    a.depth_avg = None
    assert _call(a, d) == INVALID and _err() == "fusion_filter: null pointer argument"
    a = _args(cams)
    a.src_depth[1] = None
    assert _call(a, d) == INVALID and _err() == "fusion_filter: null src_depth pointer"
    assert lib().aarmvs_fusion_filter_dedup(None, ctypes.byref(d), None) == INVALID
    assert _err() == "fusion_filter: null args"
    # without the de-duplication arguments it is aarmvs_fusion_filter, with its messages
    a = _args(cams)
    a.H = 0
    assert _call(a, None) == INVALID and _err() == "fusion_filter: need H, W >= 1 and 1 <= nsrc <= 10"
    assert lib().aarmvs_fusion_filter_dedup(None, None, None) == INVALID and _err() == "fusion_filter: null args"
    # null used maps are allowed: they pass validation (checked on the GPU), so only a later
    # check can refuse such a call
    a, d = _args(cams), _dedup()
    d.used_ref = None
    d.used_src[0] = None
    d.emit_mask = None
    assert _call(a, d) == INVALID and "emit_mask" in _err()


def test_python_surface():
    import inspect

    import torch
    from aarmvs import AarmvsError, fusion
    base = ["--test_dataset", "dtu", "--testpath", "p", "--testlist", "l", "--outdir", "o"]
    assert fusion.parse_args(base).dedup is False
    assert fusion.parse_args(base + ["--dedup"]).dedup is True
    for fn in (fusion.filter_depth, fusion.filter_depth_tnt, fusion.fuse_views):
        assert inspect.signature(fn).parameters["dedup"].default is False
    # CPU tensors are refused: there is no CPU fallback
    z = torch.zeros(4, 4)
    u = torch.zeros(4, 4, dtype=torch.uint8)
    cam = (torch.eye(3).numpy(), torch.eye(4).numpy())
    with pytest.raises(AarmvsError):
        fusion.filter_depth_dedup(z, z, cam, [z], [cam], 0.35, u, [u])
    with pytest.raises(AarmvsError, match="used maps"):
        fusion.filter_depth_dedup(z, z, cam, [z], [cam], 0.35, u, [u, u])


def test_cli_hands_dedup_to_the_driver_only_when_asked(tmp_path):
    from aarmvs import fusion
    (tmp_path / "list.txt").write_text("scan1\n")
    calls = []
    saved = fusion.filter_depth_tnt, fusion.filter_depth
    fusion.filter_depth_tnt = lambda *a, **k: calls.append(("tnt", a, k))
    fusion.filter_depth = lambda *a, **k: calls.append(("dtu", a, k))
    base = ["--testpath", "/data", "--testlist", str(tmp_path / "list.txt"), "--outdir", "/out"]
    try:
        fusion.main(["--test_dataset", "dtu"] + base)
        fusion.main(["--test_dataset", "dtu", "--dedup"] + base)
        fusion.main(["--test_dataset", "tnt", "--dedup"] + base)
    finally:
        fusion.filter_depth_tnt, fusion.filter_depth = saved
    dtu = ("/data/scan1", "/out/scan1", "/out/mvsnet_001_l3.ply", 0.35, "cuda")
    assert calls == [("dtu", dtu, {}), ("dtu", dtu, {"dedup": True}),
                     ("tnt", ("/data/scan1", "/out/scan1", "/out/scan1.ply", 0.3, "cuda"), {"dedup": True})]
