"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/soswsod_hip.h declares; every ctypes
signature and every Python copy of a header constant agrees with the header (no compute calls without a GPU); the product path
refuses to run without the library."""
import ctypes
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _header():
    src = open(os.path.join(ROOT, "include", "soswsod_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _declared_symbols():
    return sorted(set(re.findall(r"\b(sw_[a-z0-9_]+)\s*\(", _header())))


def _prototypes():
    """name -> (return type, [argument types]) as C spells them, `*` kept, qualifiers and argument names dropped"""
    src = re.sub(r"typedef\s+struct[^{;]*\{.*?\}[^;]*;", "", _header(), flags=re.S)          # struct bodies hold `;` but no prototype
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)

    def ctype(decl, named):
        decl = re.sub(r"\b(const|struct)\b", " ", decl)
        stars = "*" * decl.count("*")
        words = decl.replace("*", " ").split()
        if named and not (stars == "" and words == ["void"]):
            words = words[:-1]                                                                # the argument's name
        return " ".join(words) + stars

    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(sw_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", src):
        args = [a for a in (x.strip() for x in args.split(",")) if a]
        args = [] if args == ["void"] else [ctype(a, True) for a in args]
        assert name not in out, f"{name} declared twice"
        out[name] = (ctype(ret, False), args)
    return out


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "float": ctypes.c_float,
            "double": ctypes.c_double, "uint64_t": ctypes.c_uint64}


def _matches(c_type, ct):
    if c_type.endswith("*") or c_type == "sw_stream_t":
        return ct in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(ct, type) and issubclass(ct, ctypes._Pointer))
    return c_type in _SCALARS and ct is _SCALARS[c_type]


def _defines():
    return {k: int(v) for k, v in re.findall(r"^#define\s+(SW_\w+)\s+(\d+)\s*$", _header(), flags=re.M)}


def test_header_symbols_exported_and_bound():
    import sos_wsod_amd._lib as L
    names = _declared_symbols()
    assert len(names) >= 25
    lib = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in the header but not exported"
        assert n in L.SIGNATURES, f"{n} has no ctypes signature"
    assert set(L.SIGNATURES) == set(names)
    assert L.lib.sw_version().startswith(b"soswsod-hip")


def test_entries_without_callers_are_gone():
    """the five entries whose Python wrappers had no caller left: neither declared nor exported (the bodies gemm.hip and elementwise.hip
    still call are internal functions there)"""
    import sos_wsod_amd._lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for n in ("sw_conv3x3_wgrad_slabs", "sw_colsum_partial", "sw_colsum_fold", "sw_to_f32", "sw_decode_boxes"):
        assert n not in _declared_symbols() and n not in L.SIGNATURES, n
        assert not hasattr(lib, n), f"{n} is still exported"


def test_ctypes_signatures_match_header_prototypes():
    """argument count, every scalar's width and kind, pointer-ness and the return type of every SIGNATURES row"""
    import sos_wsod_amd._lib as L
    protos = _prototypes()
    assert set(protos) == set(_declared_symbols())                                            # the parser saw every prototype
    bad = []
    for name, (ret, args) in sorted(protos.items()):
        res, argtypes = L.SIGNATURES[name]
        if not _matches(ret, res):
            bad.append(f"{name}: returns {ret}, bound as {res.__name__}")
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} arguments in the header, {len(argtypes)} bound")
            continue
        bad += [f"{name}: argument {i} is {a}, bound as {t.__name__}" for i, (a, t) in enumerate(zip(args, argtypes))
                if not _matches(a, t)]
    assert not bad, "\n".join(bad)


def test_python_mirrors_of_header_constants():
    import sos_wsod_amd._lib as L
    import sos_wsod_amd.evaluation as E
    import sos_wsod_amd.ops as ops
    d = _defines()
    assert (L.SW_F32, L.SW_BF16) == (d["SW_F32"], d["SW_BF16"])
    assert L.SGD_MAX_TENSORS == d["SW_SGD_MAX_TENSORS"]
    assert ops.VOC_THRESHOLDS == d["SW_VOC_THRESHOLDS"] == len(E.IOU_THRESHOLDS)
    assert E.MAX_CLASSES == d["SW_VOC_MAX_CLASSES"]
    for name in ("THRESHOLDS", "RECALLS", "AREAS", "MAXDETS", "LDS_DOUBLES", "MAX_CLASSES", "WS_HEADER"):
        assert getattr(ops, "COCO_" + name) == d["SW_COCO_" + name], name
    assert (len(E.COCO_IOU_THRS), len(E.COCO_REC_THRS), len(E.COCO_AREA_RNG), len(E.COCO_MAX_DETS)) == \
        (d["SW_COCO_THRESHOLDS"], d["SW_COCO_RECALLS"], d["SW_COCO_AREAS"], d["SW_COCO_MAXDETS"])
    assert E.COCO_MAX_DETS[-1] <= d["SW_COCO_MAX_PAIR_DETS"]                                  # the evaluator's per-pair cut fits the kernel's


def test_missing_extension_fails_loudly(tmp_path, monkeypatch):
    import sos_wsod_amd._lib as L
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError):
        L.load()


def test_ops_refuse_cpu_tensors():
    import torch
    import sos_wsod_amd.ops as ops
    a = torch.zeros(8, 8)
    with pytest.raises(RuntimeError):
        ops.gemm(a, a, a, 8, 8, 8)


def test_config_reads_reference_style_yaml(tmp_path):
    from sos_wsod_amd.config import add_wsl_config, get_cfg
    base = tmp_path / "base.yaml"
    base.write_text("MODEL:\n  META_ARCHITECTURE: 'MultiInputRCNN'\n  ROI_BOX_HEAD:\n    NAME: 'DiscriminativeAdaptionNeck'\n    POOLER_RESOLUTION: 7\n")
    top = tmp_path / "top.yaml"
    top.write_text("_BASE_: 'base.yaml'\nMODEL:\n  BACKBONE:\n    NAME: 'build_vgg_backbone'\n    FREEZE_AT: 2\n  VGG:\n    CONV5_DILATION: 2\n"
                   "SOLVER:\n  STEPS: (35000, 50000)\nWSL:\n  REFINE_NUM: 4\n  REFINE_REG: [True, True, True, True]\n")
    cfg = add_wsl_config(get_cfg())
    cfg.merge_from_file(str(top))
    cfg.merge_from_list(["MODEL.AMD.COMPUTE_DTYPE", "fp32"])
    assert cfg.MODEL.META_ARCHITECTURE == "MultiInputRCNN" and cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION == 7
    assert cfg.SOLVER.STEPS == (35000, 50000) and cfg.WSL.REFINE_NUM == 4 and cfg.MODEL.VGG.CONV5_DILATION == 2
    assert cfg.MODEL.AMD.COMPUTE_DTYPE == "fp32"


def test_model_builds_from_cfg_with_reference_state_dict_names():
    """registry strings -> modules; parameter names/shapes = SURVEY A.3 (checkpoint contract)."""
    from sos_wsod_amd.config import add_wsl_config, get_cfg
    from sos_wsod_amd.rcnn_multi import build_model
    cfg = add_wsl_config(get_cfg())
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.META_ARCHITECTURE", "MultiInputRCNN", "MODEL.BACKBONE.NAME",
                         "build_vgg_backbone", "MODEL.VGG.CONV5_DILATION", 2, "MODEL.ROI_HEADS.NAME", "OICRPlusHeads",
                         "MODEL.ROI_HEADS.IN_FEATURES", ["plain5"], "MODEL.ROI_HEADS.NUM_CLASSES", 20,
                         "MODEL.ROI_HEADS.IOU_THRESHOLDS", [0.5, 0.6], "MODEL.ROI_HEADS.IOU_LABELS", [0, -1, 1],
                         "MODEL.ROI_BOX_HEAD.NAME", "DiscriminativeAdaptionNeck", "MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIPool",
                         "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7, "MODEL.ROI_BOX_HEAD.DAN_DIM", [64, 64],
                         "MODEL.PROPOSAL_GENERATOR.NAME", "PrecomputedProposals", "WSL.REFINE_NUM", 4,
                         "WSL.REFINE_REG", [True] * 4, "WSL.REFINE_MIST", True])
    model = build_model(cfg)
    sd = model.state_dict()
    assert tuple(sd["backbone.plain1.0.conv1.weight"].shape) == (64, 3, 3, 3)
    assert tuple(sd["backbone.plain5.0.conv3.weight"].shape) == (512, 512, 3, 3)
    assert tuple(sd["roi_heads.box_head.fc1.weight"].shape) == (64, 25088)
    assert tuple(sd["roi_heads.box_predictor.det.weight"].shape) == (20, 64)
    assert tuple(sd["roi_heads.box_refinery_3.bbox_pred.weight"].shape) == (80, 64)
    assert tuple(sd["roi_heads.box_refinery_0.cls_score.bias"].shape) == (21,)
    assert tuple(sd["pixel_mean"].shape) == (3, 1, 1)
    frozen = [k for k, p in model.named_parameters() if not p.requires_grad]
    assert all(k.startswith(("backbone.plain1", "backbone.plain2")) for k in frozen) and len(frozen) == 8
    n = sum(p.numel() for p in model.parameters())
    assert n == 14714688 + 64 * 25088 + 64 + 64 * 64 + 64 + 2 * (20 * 64 + 20) + 4 * (21 * 64 + 21 + 80 * 64 + 80)
