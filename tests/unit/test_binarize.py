"""``--binarize`` on the host: the numpy oracle ``bernoulli_rows`` (what kernel
binarize_rows_k must write, bit for bit), the ``Binarizer`` and the runner on
the torch backend (dynamic redraws, resume, checkpoint record)."""
import math

import numpy as np
import pytest
import torch

from multidisttorch_amd.ckpt import checkpoint as ckpt
from multidisttorch_amd.data.binarize import BINARIZE_CHOICES, Binarizer, check_mode
from multidisttorch_amd.data.datasets import synthetic_images
from multidisttorch_amd.data.sampler import shard_indices
from multidisttorch_amd.hpo import runner
from multidisttorch_amd.hpo.runner import RunOptions, run_trial
from multidisttorch_amd.hpo.trial import build_specs
from multidisttorch_amd.models.trainer_base import EVAL_STREAM
from multidisttorch_amd.ops.philox import (BINARIZE_TAG, bernoulli_rows, binarize_counter, philox4x32_10,
                                           reparam_counter)

SEED = 0x1234_5678_9ABC


@pytest.fixture(scope="module")
def grey():
    X = np.random.default_rng(0).random((40, 23), dtype=np.float32)
    X[3, :] = 0.0
    X[4, :] = 1.0
    X[5, ::2] = 0.5
    return X


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("mode", ["threshold", "static", "dynamic"])
def test_output_is_binary_and_extremes_are_fixed(grey, mode):
    idx = np.arange(40)
    for epoch in range(6):
        for split in (0, 1):
            out = bernoulli_rows(grey, idx, SEED + epoch, epoch, split, mode)
            assert out.dtype == np.float32 and out.shape == grey.shape
            assert np.isin(out, (0.0, 1.0)).all()
            assert (out[3] == 0).all() and (out[4] == 1).all()  # x = 0 never fires, x = 1 always


def test_draw_is_keyed_by_the_global_row(grey):
    full = bernoulli_rows(grey, np.arange(40), SEED, 7, 0, "dynamic")
    sub = np.array([31, 2, 17, 2, 39, 0])  # another order, a subset, a repeated row
    np.testing.assert_array_equal(bernoulli_rows(grey, sub, SEED, 7, 0, "dynamic"), full[sub])
    np.testing.assert_array_equal(bernoulli_rows(grey, sub[:1], SEED, 7, 0, "dynamic"), full[sub[:1]])


def test_epoch_split_and_seed_change_the_bits(grey):
    idx = np.arange(40)
    base = bernoulli_rows(grey, idx, SEED, 1, 0, "dynamic")
    np.testing.assert_array_equal(base, bernoulli_rows(grey, idx, SEED, 1, 0, "dynamic"))
    assert (base != bernoulli_rows(grey, idx, SEED, 2, 0, "dynamic")).any()
    assert (base != bernoulli_rows(grey, idx, SEED, 1, 1, "dynamic")).any()
    assert (base != bernoulli_rows(grey, idx, SEED + 1, 1, 0, "dynamic")).any()
    assert (base != bernoulli_rows(grey, idx, SEED + (1 << 32), 1, 0, "dynamic")).any()  # the high key word counts


def test_threshold_ignores_the_seed(grey):
    idx = np.arange(40)
    a = bernoulli_rows(grey, idx, 1, 0, 0, "threshold")
    np.testing.assert_array_equal(a, bernoulli_rows(grey, idx, 99, 5, 1, "threshold"))
    np.testing.assert_array_equal(a, (grey >= 0.5).astype(np.float32))
    assert (a[5, ::2] == 1).all()  # 0.5 itself is on


def test_word_j_serves_pixel_4q_plus_j():
    """One pixel recomputed by hand from the documented counter layout."""
    X = np.full((9, 11), 0.5, np.float32)
    out = bernoulli_rows(X, [6], SEED, 3, 1, "dynamic")
    for p in range(11):
        c = binarize_counter(p, 6, 3, 1)
        assert c == (p // 4, 6, 3, BINARIZE_TAG | 1)
        w = philox4x32_10(np.array([c[0]], np.uint32), c[1], c[2], c[3], SEED & 0xFFFFFFFF, SEED >> 32)
        u = np.float32(int(w[p % 4][0]) >> 8) * np.float32(2.0 ** -24)
        assert 0.0 <= u < 1.0 and out[0, p] == (1.0 if u < 0.5 else 0.0)


def test_unbiased_over_epochs():
    """64 pixels on a grid of probabilities, n = 4096 epochs: every pixel's mean
    within 6 binomial standard deviations of p (+ the 2^-24 grid of u)."""
    n = 4096
    p = (np.arange(64, dtype=np.float32) / np.float32(63))[None, :]
    acc = np.zeros(64)
    for e in range(n):
        acc += bernoulli_rows(p, [0], SEED, e, 0, "dynamic")[0]
    mean = acc / n
    pd = p[0].astype(np.float64)
    bound = 6 * np.sqrt(pd * (1 - pd) / n) + 2.0 ** -24
    assert (np.abs(mean - pd) <= bound).all(), (np.abs(mean - pd) - bound).max()


def test_counter_never_meets_a_noise_stream():
    """Same key, so the counters must differ: binarize's fourth word is
    TAG | split (non-zero high bits), a noise draw's is step >> 32 = 0 for any
    step < 2^32, whatever the stream word is."""
    assert BINARIZE_TAG >> 16 != 0 and BINARIZE_TAG & 1 == 0
    row = 17
    for e in (0, 5, 1 << 20):  # q = e: the first words agree
        for split in (0, 1):
            for epoch in (0, 1, 17):
                b = binarize_counter(4 * e, row, epoch, split)
                assert b[0] == e
                # the nearest miss: stream = row, step_lo = epoch
                for stream in (row, 0, 1, EVAL_STREAM, EVAL_STREAM + 1, 3 << 28, 2 << 28):
                    for step in (epoch, 0, 1, (1 << 32) - 1):
                        r = reparam_counter(e, stream, step)
                        assert r[3] == 0 and b != r


def test_oracle_rejects_bad_arguments(grey):
    with pytest.raises(ValueError):
        bernoulli_rows(grey, [0], 0, 0, 0, "bernoulli")
    with pytest.raises(ValueError):
        bernoulli_rows(grey, [0], 0, 0, 2, "static")
    with pytest.raises(ValueError):
        bernoulli_rows(grey, [0], 0, 1 << 32, 0, "dynamic")
    with pytest.raises(IndexError):
        bernoulli_rows(grey, [40], 0, 0, 0, "dynamic")


# ------------------------------------------------------------------ Binarizer
def test_binarizer_modes(grey):
    X = torch.from_numpy(grey)
    idx = torch.tensor([9, 1, 30, 1], dtype=torch.int32)
    for mode in ("static", "threshold"):
        b = Binarizer(mode, SEED, X, idx, 0)
        assert b.refresh(1) and b.data.shape == (4, 23) and len(b) == 4
        first, ptr = b.data.clone(), b.data.data_ptr()
        assert not b.refresh(2)
        assert torch.equal(b.data, first) and b.data.data_ptr() == ptr
        np.testing.assert_array_equal(first.numpy(), bernoulli_rows(grey, idx.numpy(), SEED, 0, 0, mode))
        assert torch.equal(b.index(), torch.arange(4, dtype=torch.int32))
    d = Binarizer("dynamic", SEED, X, idx, 0)
    d.refresh(1)
    first, ptr = d.data.clone(), d.data.data_ptr()
    assert d.refresh(2) and d.data.data_ptr() == ptr  # rewritten in place
    assert not torch.equal(d.data, first)
    np.testing.assert_array_equal(d.data.numpy(), bernoulli_rows(grey, idx.numpy(), SEED, 2, 0, "dynamic"))
    assert d.refresh(1) and torch.equal(d.data, first)  # the epoch is the key: a redraw repeats


def test_test_split_ignores_the_epoch(grey):
    X = torch.from_numpy(grey)
    idx = torch.arange(40, dtype=torch.int32)
    t = Binarizer("dynamic", SEED, X, idx, 1)
    t.refresh(1)
    first = t.data.clone()
    t.refresh(5)
    assert torch.equal(t.data, first)
    np.testing.assert_array_equal(first.numpy(), bernoulli_rows(grey, idx.numpy(), SEED, 0, 1, "dynamic"))
    tr = Binarizer("dynamic", SEED, X, idx, 0)
    tr.refresh(0)
    assert not torch.equal(tr.data, first)  # train and test never share a draw


def test_bad_mode_names_raise_at_start_up(grey):
    X = torch.from_numpy(grey)
    idx = torch.arange(4, dtype=torch.int32)
    for bad in ("none", "bernoulli", "", "Dynamic"):
        with pytest.raises(ValueError, match="binarize mode"):
            Binarizer(bad, 0, X, idx, 0)
    with pytest.raises(ValueError):
        check_mode("fixed")
    assert check_mode("none") == "none" and BINARIZE_CHOICES == ("none", "threshold", "static", "dynamic")
    with pytest.raises(IndexError):
        Binarizer("static", 0, X, torch.tensor([40], dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="binarize mode"):  # before any data is loaded or trainer built
        run_trial(build_specs(1, 1, None, None, 0)[0], None, RunOptions(binarize="bernoulli"))


def test_train_data_changed_is_part_of_the_trainer_api():
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
    from multidisttorch_amd.models.trainer_base import VaeTrainerBase

    assert "rewritten in place" in VaeTrainerBase.train_data_changed.__doc__
    assert MlpVaeTrainer.train_data_changed is VaeTrainerBase.train_data_changed
    assert ConvVaeTrainer.train_data_changed is not VaeTrainerBase.train_data_changed
    tr = MlpVaeTrainer(batch_size=8, D=16, H=8, Z=2, backend="torch")
    assert tr.train_data_changed() is None


# ------------------------------------------------------------------ runner, torch backend
B, N_TRAIN, N_TEST = 96, 512, 256  # 5 whole batches + a tail of 32


def _opts(model, **kw):
    return RunOptions(batch_size=B, backend="torch", results=False, synthetic=True, train_samples=N_TRAIN,
                      test_samples=N_TEST, model=model, quiet_train_log=True, **kw)


@pytest.fixture(scope="module")
def data():
    from multidisttorch_amd.data.datasets import ImageSet

    tr = synthetic_images(N_TRAIN, seed=0)
    te = synthetic_images(N_TEST, seed=1)
    return ImageSet(tr, (1, 28, 28), True, "synthetic28"), ImageSet(te, (1, 28, 28), True, "synthetic28")


def _run(monkeypatch, spec, opts, data):
    """run_trial, returning (result, the trainer it built)."""
    made = []
    real = runner._make_trainer

    def spy(*a, **kw):
        made.append(real(*a, **kw))
        return made[-1]

    monkeypatch.setattr(runner, "_make_trainer", spy)
    res = run_trial(spec, None, opts, data=data)
    monkeypatch.setattr(runner, "_make_trainer", real)
    assert not res.failed, res.error
    return res, made[-1]


@pytest.mark.parametrize("model", ["mlp", "conv"])
def test_run_trial_dynamic_equals_hand_driven_oracle_rows(monkeypatch, data, capsys, model):
    spec = build_specs(1, 2, None, None, 11)[0]
    opts = _opts(model, binarize="dynamic")
    res, got = _run(monkeypatch, spec, opts, data)
    assert res.epochs == 2
    train, test = data
    idx = shard_indices(N_TRAIN, 1, 0)
    assert idx.numel() == N_TRAIN
    ref = runner._make_trainer(spec, opts, torch.device("cpu"), 0, 784, runner._total_steps(spec, opts, N_TRAIN))
    for epoch in (1, 2):
        rows = torch.from_numpy(bernoulli_rows(train.data.numpy(), idx.numpy(), spec.seed, epoch, 0, "dynamic"))
        ref.bind_train_data(rows, torch.arange(N_TRAIN, dtype=torch.int32))
        ref.set_cursor(0, 6)
        ref.reset_loss()
        ref.train_steps(5, B)
        ref.train_steps(1, N_TRAIN % B)
    assert ref.step_count == got.step_count == 12
    assert torch.equal(got.params, ref.params)
    assert torch.equal(got.exp_avg, ref.exp_avg) and torch.equal(got.exp_avg_sq, ref.exp_avg_sq)
    # the test loss the trial printed is over the fixed binarized test set
    tb = torch.from_numpy(bernoulli_rows(test.data.numpy(), np.arange(N_TEST), spec.seed, 0, 1, "dynamic"))
    ti = torch.arange(N_TEST, dtype=torch.int32)
    ref.evaluate(tb, ti, want_first_recon=False)  # epoch 1's pass: the eval noise is keyed by the eval step
    total, _ = ref.evaluate(tb, ti, want_first_recon=False)
    assert res.final_test_loss == total / N_TEST
    ref._st_eval["step"] -= 3  # the same noise again, over the grey levels
    grey_total, _ = ref.evaluate(test.data, ti, want_first_recon=False)
    assert abs(grey_total - total) > 1e-3 * total
    capsys.readouterr()


@pytest.mark.parametrize("model", ["mlp", "conv"])
def test_resume_redraws_what_an_uninterrupted_trial_would(monkeypatch, data, tmp_path, capsys, model):
    straight = _run(monkeypatch, build_specs(1, 2, None, None, 5)[0], _opts(model, binarize="dynamic"), data)[1]
    ck = str(tmp_path / "ck")
    _run(monkeypatch, build_specs(1, 1, None, None, 5)[0], _opts(model, binarize="dynamic", ckpt_dir=ck), data)
    raw = torch.load(ckpt.latest_path(ck, 0), weights_only=True)
    assert raw["data"] == {"binarize": "dynamic"}
    res, resumed = _run(monkeypatch, build_specs(1, 2, None, None, 5)[0],
                        _opts(model, binarize="dynamic", ckpt_dir=ck, resume=True), data)
    assert res.epochs == 1 and "resumed trial 0" in capsys.readouterr().out
    assert torch.equal(resumed.params, straight.params)
    assert torch.equal(resumed.exp_avg, straight.exp_avg) and torch.equal(resumed.exp_avg_sq, straight.exp_avg_sq)


def test_resume_under_another_binarize_raises(monkeypatch, data, tmp_path, capsys):
    ck = str(tmp_path / "ck")
    spec = build_specs(1, 1, None, None, 5)[0]
    _run(monkeypatch, spec, _opts("mlp", binarize="static", ckpt_dir=ck), data)
    for other in ("none", "dynamic"):
        with pytest.raises(ValueError, match="--binarize static"):
            run_trial(build_specs(1, 2, None, None, 5)[0], None,
                      _opts("mlp", binarize=other, ckpt_dir=ck, resume=True), data=data)
    # a checkpoint without the entry counts as none
    path = ckpt.latest_path(ck, 0)
    raw = torch.load(path, weights_only=True)
    del raw["data"]
    torch.save(raw, path)
    tr = runner._make_trainer(spec, _opts("mlp"), torch.device("cpu"), 0, 784, 6)
    assert ckpt.load_latest(ck, 0, tr)["binarize"] == "none"
    with pytest.raises(ValueError, match="--binarize none"):
        run_trial(build_specs(1, 2, None, None, 5)[0], None, _opts("mlp", binarize="static", ckpt_dir=ck, resume=True),
                  data=data)
    capsys.readouterr()


def test_default_run_writes_none_and_logs_no_binarize_time(monkeypatch, data, tmp_path, capsys):
    import json

    ck, md = str(tmp_path / "ck"), str(tmp_path / "m")
    spec = build_specs(1, 1, None, None, 5)[0]
    _run(monkeypatch, spec, _opts("mlp", ckpt_dir=ck, metrics_dir=md, profile=True), data)
    assert torch.load(ckpt.latest_path(ck, 0), weights_only=True)["data"] == {"binarize": "none"}
    rec = [json.loads(l) for l in open(tmp_path / "m" / "trial-0.jsonl")]
    assert all("binarize_s" not in r for r in rec)
    md2 = str(tmp_path / "m2")
    _run(monkeypatch, spec, _opts("mlp", binarize="dynamic", metrics_dir=md2, profile=True), data)
    rec = [json.loads(l) for l in open(tmp_path / "m2" / "trial-0.jsonl") if "epoch" in json.loads(l)]
    assert rec and all(r["binarize_s"] >= 0 and math.isfinite(r["binarize_s"]) for r in rec)
    md3 = str(tmp_path / "m3")
    _run(monkeypatch, spec, _opts("mlp", binarize="dynamic", metrics_dir=md3), data)
    assert all("binarize_s" not in json.loads(l) for l in open(tmp_path / "m3" / "trial-0.jsonl"))
    capsys.readouterr()


def test_packed_trials_binarize_per_trial(monkeypatch, data, capsys):
    """Two packed trials: each redraws its own shard under its own seed and
    matches the same trial run alone on that shard."""
    from multidisttorch_amd.hpo.runner import run_packed_trials

    specs = build_specs(2, 1, None, None, 21, epoch_offset=False)
    made = []
    real = runner._make_trainer

    def spy(*a, **kw):
        made.append(real(*a, **kw))
        return made[-1]

    monkeypatch.setattr(runner, "_make_trainer", spy)
    res = run_packed_trials(specs, None, _opts("mlp", binarize="dynamic"), data=data, num_trials=2)
    monkeypatch.setattr(runner, "_make_trainer", real)
    assert [r.failed for r in res] == [False, False] and [r.shard for r in res] == [256, 256]
    train, _ = data
    for spec, got in zip(specs, made):
        idx = shard_indices(N_TRAIN, 2, spec.group_id)
        rows = torch.from_numpy(bernoulli_rows(train.data.numpy(), idx.numpy(), spec.seed, 1, 0, "dynamic"))
        ref = real(spec, _opts("mlp"), torch.device("cpu"), 0, 784, 3)
        ref.bind_train_data(rows, torch.arange(256, dtype=torch.int32))
        ref.set_cursor(0, 3)
        ref.train_steps(2, B)
        ref.train_steps(1, 256 % B)
        assert torch.equal(got.params, ref.params)
    assert not torch.equal(made[0].params, made[1].params)
    capsys.readouterr()
