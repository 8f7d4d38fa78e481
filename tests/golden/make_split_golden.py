"""Generate tests/golden/split_files.npz by RUNNING the reference's split tools (/root/reference/unbias/split_single.py main(),
generate_base_split.py as __main__) and the Stage-3 loader's divide_label_unlabel (unbias/ubteacher/data/build.py:33-56) on
synthetic inputs — build container only:

    python tests/golden/make_split_golden.py [OUT_DIR]          (default: tests/golden)

detectron2 / ubteacher are stubbed: build_model returns a model whose forward returns the recorded loss of the image it is given
(as loss_cls; the three other losses 0), build_detection_train_loader a dataset of {"image_id": i}, get_detection_dataset_dicts a
list of the case's length; torch.load returns an empty checkpoint, tqdm is the identity.  The losses are distinct (the reference's
sort is unstable: ties are this project's own rule, tested apart) with NaNs only where they sort past k.  Only (length, k) pairs
whose percent bisection ends are run (the reference loops forever on the others, split_single.py:108).

Fixture keys: per loss case c: loss_{c} (f32 losses), k_{c}, file_{c} (the bytes split_single wrote, u8), pct_{c} (its printed
line); per base length n: base_{n} (the bytes generate_base_split wrote); divide_*: divide_label_unlabel's labelled / unlabelled
dataset indices for the voc case's file."""
import ast
import contextlib
import io
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference/unbias"
HERE = os.path.dirname(os.path.abspath(__file__))

LOSS_CASES = {"voc07": (5011, 2000), "small": (10, 3), "k0": (37, 0), "kall": (64, 64), "coco": (117266, 2000),
              "odd": (997, 123)}
BASE_LENGTHS = (1, 2, 10, 100, 5011, 9963, 11540, 117266)


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Node(types.SimpleNamespace):
    def __getattr__(self, k):                     # any missing node is an empty node
        v = _Node()
        setattr(self, k, v)
        return v


class _Cfg(_Node):
    def merge_from_file(self, f):
        pass

    def freeze(self):
        pass

    def defrost(self):
        pass


STATE = {}


class _Model:
    def load_state_dict(self, sd, strict=True):
        return "<All keys matched successfully>"

    def __call__(self, data):
        v = torch.tensor(STATE["losses"][int(data[0]["image_id"])], dtype=torch.float32)
        z = torch.zeros((), dtype=torch.float32)
        return {"loss_cls": v, "loss_box_reg": z, "loss_rpn_cls": z, "loss_rpn_loc": z}, None, None, None


def _install_stubs():
    class _Loader:
        def __init__(self, n):
            self.dataset = types.SimpleNamespace(dataset=[{"image_id": i} for i in range(n)])

    _mod("tqdm", tqdm=lambda x, *a, **k: x)
    _mod("detectron2"); _mod("detectron2.config", get_cfg=_Cfg); _mod("detectron2.modeling", build_model=lambda cfg: _Model())
    _mod("detectron2.data", build_detection_train_loader=lambda cfg: _Loader(STATE["n"]),
         get_detection_dataset_dicts=lambda names: [{}] * STATE["n"])
    _mod("detectron2.utils"); _mod("detectron2.utils.events", EventStorage=contextlib.nullcontext)
    _mod("ubteacher", add_ubteacher_config=lambda cfg: None)
    for n in ("ubteacher.modeling", "ubteacher.modeling.meta_arch", "ubteacher.modeling.proposal_generator", "ubteacher.modeling.roi_heads"):
        _mod(n)
    _mod("ubteacher.modeling.meta_arch.rcnn", TwoStagePseudoLabGeneralizedRCNN=None)
    _mod("ubteacher.modeling.proposal_generator.rpn", PseudoLabRPN=None)
    _mod("ubteacher.modeling.roi_heads.roi_heads", StandardROIHeadsPseudoLab=None)


def _terminates(length, k):
    low, high = k / length, (k + 1) / length
    for _ in range(200):
        middle = round((low + high) / 2, 7)
        val = int(length * middle)
        if val == k:
            return True
        if val < k:
            return False
        high = middle
    return False


def _losses(n, tag):
    rng = np.random.default_rng([n, sum(map(ord, tag))])
    v = rng.permutation(n).astype(np.float64) * 0.001 + rng.random(n) * 1e-4 + 0.05     # distinct after the f32 cast
    v = v.astype(np.float32)
    assert len(np.unique(v)) == n
    return v


def _divide_fn():
    src = open(os.path.join(REF, "ubteacher", "data", "build.py")).read()
    tree = ast.parse(src)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "divide_label_unlabel"][0]
    ns = {"np": np, "json": json}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "build.py", "exec"), ns)
    return ns["divide_label_unlabel"]


def main(out_dir):
    _install_stubs()
    orig_load, orig_argv = torch.load, sys.argv
    torch.load = lambda *a, **k: {"model": {"modelStudent.x": 0, "modelTeacher.x": 0}}
    sys.path.insert(0, REF)
    spec = runpy.run_path(os.path.join(REF, "split_single.py"), run_name="split_single_ref")
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for name, (n, k) in LOSS_CASES.items():
            assert _terminates(n, k), name
            losses = _losses(n, name)
            if name == "odd":                        # NaNs: they sort last (torch.sort), all beyond k
                losses[[3, 500, 996]] = np.nan
            STATE.update(n=n, losses=losses)
            out = os.path.join(td, f"{name}.txt")
            sys.argv = ["split_single.py", "--config", "x.yaml", "--ckpt", "x.pth", "--save-path", out, "--k", str(k)]
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                spec["main"]()
            line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("The finded percent is")][0]
            res[f"loss_{name}"] = losses; res[f"k_{name}"] = np.int64(k)
            res[f"file_{name}"] = np.frombuffer(open(out, "rb").read(), dtype=np.uint8)
            res[f"pct_{name}"] = np.array(line)
        for n in BASE_LENGTHS:
            STATE.update(n=n)
            out = os.path.join(td, f"base_{n}.txt")
            sys.argv = ["generate_base_split.py", "--config", "x.yaml", "--save-path", out]
            runpy.run_path(os.path.join(REF, "generate_base_split.py"), run_name="__main__")
            res[f"base_{n}"] = np.frombuffer(open(out, "rb").read(), dtype=np.uint8)
        divide = _divide_fn()
        seed_path = os.path.join(td, "voc07.txt")
        with open(seed_path, "wb") as f:
            f.write(res["file_voc07"].tobytes())
        pct = float(list(json.loads(res["file_voc07"].tobytes()))[0])
        dicts = [{"i": i} for i in range(5011)]
        lab, unl = divide(dicts, pct, 1, seed_path)
        res["divide_pct"] = np.float64(pct)
        res["divide_label"] = np.array([d["i"] for d in lab], dtype=np.int32)
        res["divide_unlabel"] = np.array([d["i"] for d in unl], dtype=np.int32)
    torch.load, sys.argv = orig_load, orig_argv
    path = os.path.join(out_dir, "split_files.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
