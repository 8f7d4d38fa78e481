"""bench.py --dump-outputs on the benchmarked model's parameters — host logic, runs without a GPU."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_writes_the_losses_and_a_fixed_sample_of_every_trainable_parameter(tmp_path):
    model = bench.build("cpu", torch.float32)
    losses = {"loss_cls": torch.tensor(0.5), "loss_box_reg_r0": torch.tensor(0.25, dtype=torch.bfloat16)}
    bench.dump_outputs(str(tmp_path / "a"), losses, model)
    bench.dump_outputs(str(tmp_path / "b"), losses, model)
    trainable = {n: p.detach() for n, p in model.named_parameters() if p.requires_grad}
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted([f"{k}.npy" for k in losses] + [f"param.{n}.npy" for n in trainable])
    total = 0
    for f in names:
        a = np.load(tmp_path / "a" / f)
        total += a.nbytes
        assert a.dtype == np.float32 and np.array_equal(a, np.load(tmp_path / "b" / f)), f      # same sample in every run
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "loss_cls.npy") == 0.5 and np.load(tmp_path / "a" / "loss_box_reg_r0.npy") == 0.25
    bias = trainable["roi_heads.box_head.fc1.bias"]                  # small tensors: whole
    assert np.array_equal(np.load(tmp_path / "a" / "param.roi_heads.box_head.fc1.bias.npy"), bias.numpy())
    w = trainable["roi_heads.box_predictor.cls.weight"].reshape(-1).numpy()       # 81920 elements: a sample of them
    s = np.load(tmp_path / "a" / "param.roi_heads.box_predictor.cls.weight.npy")
    assert s.shape == (bench.DUMP_SAMPLE,) and np.isin(s, w).all()
