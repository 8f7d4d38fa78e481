"""One run of `python -m sos_wsod_amd.split loss` for tests/test_gpu_split.py: as a plain process (one rank) or under
torch.distributed.run (two ranks sharing cuda:0 over gloo).  argv: config yaml, checkpoint, dataset-dicts json, output path,
images per batch.  The images are PNG files the dicts name, decoded by the CLI's own Pillow loader."""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    cfg, ckpt, dicts_path, out, ipb = sys.argv[1:6]
    import sos_wsod_amd  # noqa: F401
    from sos_wsod_amd import split
    with open(dicts_path) as f:
        dicts = json.load(f)
    split.main(["loss", "--config", cfg, "--ckpt", ckpt, "--save-path", out, "--k", "3", "--images-per-batch", ipb, "--seed", "4"],
               dataset_dicts=dicts)


if __name__ == "__main__":
    main()
