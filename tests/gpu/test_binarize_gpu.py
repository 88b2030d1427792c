"""``--binarize`` on the MI355X: kernel binarize_rows_k against the numpy oracle
(bit for bit), the in-place rewrite under captured step graphs and the conv28
next-batch prefetch, the evaluation passes on the binarized test set, and one
run of vae-hpo.py."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from multidisttorch_amd.data.binarize import Binarizer
from multidisttorch_amd.ops.philox import bernoulli_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SEED = 0x5EED_0000_0007  # both key words in use
MODES = ("threshold", "static", "dynamic")


def _dev():
    return torch.device("cuda", 0)


def _grey(n, D, seed=0):
    X = torch.rand(n, D, generator=torch.Generator().manual_seed(seed))
    X[0, :] = 0.0
    X[-1, :] = 1.0
    X[n // 2, ::3] = 0.5
    return X


def _check(C, X, idx, epoch=3, split=0, out=None):
    """Every mode: kernel rows == oracle rows, exactly. X: device [N, D]; idx: host int list."""
    idx_d = torch.tensor(idx, dtype=torch.int32, device=X.device)
    out = torch.full((len(idx), X.shape[1]), -7.0, device=X.device) if out is None else out
    Xh = X.cpu().numpy()
    for mode in MODES:
        out.fill_(-7.0)
        C.binarize_rows(X, idx_d, out, SEED, epoch if mode == "dynamic" else 0, split, mode)
        torch.cuda.synchronize()
        want = bernoulli_rows(Xh, idx, SEED, epoch if mode == "dynamic" else 0, split, mode)
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=mode)


def test_vector_path_shuffled_subset_with_a_repeated_row(native_ext):
    X = _grey(256, 784).to(_dev())
    idx = torch.randperm(256, generator=torch.Generator().manual_seed(1))[:36].tolist()
    idx.insert(20, idx[3])
    assert len(idx) == 37
    _check(native_ext, X, idx)
    _check(native_ext, X, idx, epoch=0, split=1)


@pytest.mark.parametrize("D", [7, 5, 1])
def test_scalar_path_rows_not_16_byte_aligned(native_ext, D):
    X = _grey(9, D).to(_dev())
    _check(native_ext, X, [8, 0, 4, 4, 2])


def test_grid_stride_loop(native_ext):
    X = _grey(6, 16384).to(_dev())
    _check(native_ext, X, [5, 0, 3])
    # 130 x 4096 groups of four pixels > 2048 blocks x 256 threads: the capped grid strides
    big = _grey(130, 16384, seed=2).to(_dev())
    _check(native_ext, big, list(range(129, -1, -1)))


def test_row_word_is_not_truncated_to_16_bits(native_ext):
    idx = [0, 65535, 65536, 69999]
    X = torch.rand(70000, 8, generator=torch.Generator().manual_seed(3))
    X[[0, 65536]] = 0.5  # rows 0 and 65536 differ by their row word alone
    _check(native_ext, X.to(_dev()), idx, epoch=1)
    want = bernoulli_rows(X.numpy(), idx, SEED, 1, 0, "dynamic")
    assert not np.array_equal(want[0], want[2])  # so a 16-bit row word could not pass the comparison above


def test_alignment_fallback(native_ext):
    flat = torch.rand(1 + 20 * 784, generator=torch.Generator().manual_seed(4)).to(_dev())
    X = flat[1:].view(20, 784)
    assert X.data_ptr() % 16 == 4 and X.is_contiguous()
    idx = [19, 3, 3, 0, 7]
    _check(native_ext, X, idx)
    # and a misaligned output with an aligned input
    oflat = torch.empty(1 + 5 * 784, device=_dev())
    _check(native_ext, flat[:20 * 784].view(20, 784), idx, out=oflat[1:].view(5, 784))


def test_aliased_output_and_bad_arguments_raise(native_ext):
    C = native_ext
    X = _grey(16, 784).to(_dev())
    idx = torch.arange(4, dtype=torch.int32, device=_dev())
    with pytest.raises(ValueError, match="aliases"):
        C.binarize_rows(X, idx, X[:4], SEED, 0, 0, "dynamic")
    with pytest.raises(ValueError, match="aliases"):
        C.binarize_rows(X, idx, X[8:12], SEED, 0, 0, "threshold")
    out = torch.empty(4, 784, device=_dev())
    with pytest.raises(ValueError, match="unknown mode"):
        C.binarize_rows(X, idx, out, SEED, 0, 0, "bernoulli")
    with pytest.raises(ValueError, match="split"):
        C.binarize_rows(X, idx, out, SEED, 0, 2, "static")
    with pytest.raises(RuntimeError, match="epoch"):
        C.binarize_rows(X, idx, out, SEED, 1 << 32, 0, "dynamic")
    with pytest.raises(RuntimeError, match="out must be"):
        C.binarize_rows(X, idx, out[:3], SEED, 0, 0, "dynamic")
    # the limits of the counter words, by name (no tensor of that size is needed)
    with pytest.raises(ValueError, match=r"2\^32 range of the pixel-group counter word"):
        C.binarize_check(1, 1 << 35, 1, "dynamic", 0)
    with pytest.raises(ValueError, match=r"2\^31 rows"):
        C.binarize_check(1, 8, (1 << 31) + 1, "dynamic", 0)
    with pytest.raises(ValueError, match=r"2\^62 elements"):
        C.binarize_check(1 << 40, 1 << 30, 1 << 31, "dynamic", 0)
    C.binarize_check(0, 1, 1, "threshold", 1)


def test_enqueue_under_graph_capture_replays_to_the_same_bits(native_ext):
    C = native_ext
    X = _grey(64, 784).to(_dev())
    idx = torch.randperm(64, generator=torch.Generator().manual_seed(5))[:33].to(torch.int32).to(_dev())
    out = torch.zeros(33, 784, device=_dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        C.binarize_rows(X, idx, out, SEED, 9, 0, "dynamic")
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        C.binarize_rows(X, idx, out, SEED, 9, 0, "dynamic")
    want = bernoulli_rows(X.cpu().numpy(), idx.cpu().numpy(), SEED, 9, 0, "dynamic")
    for _ in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------ trainers
B, NB = 32, 6


def _make(kind, graphs, seed=7):
    if kind == "conv":
        from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

        return ConvVaeTrainer(batch_size=B, image=28, z=32, device=_dev(), backend="hip", seed=seed,
                              use_graphs=graphs, graph_steps=3)
    from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

    return MlpVaeTrainer(batch_size=B, device=_dev(), backend="hip", seed=seed, use_graphs=graphs, graph_steps=3)


@pytest.fixture(scope="module")
def shard():
    """Grey rows, the shard's index list and the oracle's rows of epochs 1 and 2 (shared, never written)."""
    from multidisttorch_amd.data.datasets import synthetic_images

    X = synthetic_images(256, seed=6, device=_dev())
    idx = torch.randperm(256, generator=torch.Generator().manual_seed(7))[:B * NB].to(torch.int32).to(_dev())
    Xh, ih = X.cpu().numpy(), idx.cpu().numpy()
    rows = {e: torch.from_numpy(bernoulli_rows(Xh, ih, SEED, e, 0, "dynamic")).to(_dev()) for e in (1, 2)}
    return X, idx, rows


def _arange(n):
    return torch.arange(n, dtype=torch.int32, device=_dev())


@pytest.mark.parametrize("kind", ["conv", "mlp"])
def test_step_graphs_survive_the_in_place_rewrite(native_ext, shard, kind):
    X, idx, rows = shard
    b = Binarizer("dynamic", SEED, X, idx, 0)
    tr = _make(kind, graphs=True)
    tr.bind_train_data(b.data, b.index())
    graphs = None
    for e in (1, 2):
        assert b.refresh(e)
        tr.train_data_changed()
        tr.set_cursor(0, NB)
        tr.train_steps(NB)
        torch.cuda.synchronize()
        if graphs is None:
            graphs = dict(tr._graphs)
            assert graphs
    # no graph was captured again: the same keys, the same objects
    assert tr._graphs.keys() == graphs.keys() and all(tr._graphs[k] is g for k, g in graphs.items())
    assert torch.equal(b.data, rows[2])
    ref = _make(kind, graphs=False)
    for e in (1, 2):
        ref.bind_train_data(rows[e].clone(), _arange(B * NB))
        ref.set_cursor(0, NB)
        ref.train_steps(NB)
    torch.cuda.synchronize()
    assert tr.step_count == ref.step_count == 2 * NB
    assert torch.equal(tr.params, ref.params)
    assert torch.equal(tr.exp_avg, ref.exp_avg) and torch.equal(tr.exp_avg_sq, ref.exp_avg_sq)
    np.testing.assert_array_equal(tr.loss_history()[:2 * NB], ref.loss_history()[:2 * NB])


def test_train_data_changed_drops_the_prefetched_rows(native_ext, shard):
    """conv28 with the next-batch prefetch: 3 steps, the bound rows rewritten
    in place, ``train_data_changed()``, 1 step -- and no ``set_cursor`` -- is
    bitwise a twin that trained the same 3 steps and had the new rows bound
    fresh. Without the call the fourth step trains on the rows gathered before
    the rewrite."""
    X, idx, rows = shard

    def three_steps():
        b = Binarizer("dynamic", SEED, X, idx, 0)
        tr = _make("conv", graphs=True)
        assert tr.f28 and tr.f28_prefetch
        b.refresh(1)
        tr.bind_train_data(b.data, b.index())
        tr.prepare([B])  # both step graphs exist: no capture (and its warm-up step) between the steps below
        tr.strict_graphs = True
        tr.set_cursor(0, NB)
        tr.train_steps(3)
        return b, tr

    b, tr = three_steps()
    b.refresh(2)
    tr.train_data_changed()
    tr.train_steps(1)
    b2, stale = three_steps()
    b2.refresh(2)
    stale.train_steps(1)  # the hook left out
    _, twin = three_steps()
    twin.strict_graphs = False  # a fresh binding drops the graphs
    twin.bind_train_data(rows[2].clone(), _arange(B * NB))
    twin.train_steps(1)
    torch.cuda.synchronize()
    assert tr.read_state()["step"] == twin.read_state()["step"] == 4
    assert tr.read_state()["cursor"] == twin.read_state()["cursor"] == 4
    assert torch.equal(tr.params, twin.params)
    assert torch.equal(tr.exp_avg, twin.exp_avg) and torch.equal(tr.exp_avg_sq, twin.exp_avg_sq)
    np.testing.assert_array_equal(tr.loss_history()[:4], twin.loss_history()[:4])
    assert not torch.equal(stale.params, twin.params)


@pytest.mark.parametrize("kind", ["conv", "mlp"])
def test_evaluation_reads_the_binarized_test_set(native_ext, kind):
    from multidisttorch_amd.data.datasets import synthetic_images

    n = 85
    T = synthetic_images(n, seed=8, device=_dev())
    bt = Binarizer("dynamic", SEED, T, torch.arange(n, dtype=torch.int32), 1)
    bt.refresh(4)  # a test split ignores the epoch
    want = torch.from_numpy(bernoulli_rows(T.cpu().numpy(), np.arange(n), SEED, 0, 1, "dynamic")).to(_dev())
    assert torch.equal(bt.data, want)
    tr = _make(kind, graphs=True)
    res = []
    for rows in (bt.data, want, T):
        tr.state.set_step(True, 0)  # the eval noise is keyed by the eval step: the same draws for every pass
        total, first = tr.evaluate(rows, _arange(n), want_first_recon=True)
        iw = tr.evaluate_iw(rows, _arange(n), 5)
        res.append((total, first.clone(), iw["nll"], iw["neg_elbo"]))
    a, o, grey = res
    assert a[0] == o[0] and torch.equal(a[1], o[1]) and a[2] == o[2] and a[3] == o[3]
    assert np.isfinite([a[0], a[2], a[3]]).all()
    assert a[0] != grey[0] and a[2] != grey[2]


def test_vae_hpo_binarize_dynamic_conv(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vae-hpo.py"), "--ngroups", "1", "--model", "conv",
                        "--binarize", "dynamic", "--iw-samples", "5", "--epochs", "2", "--synthetic",
                        "--train-samples", "512", "--test-samples", "256", "--metrics-dir", "m", "--profile"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    text = r.stdout + r.stderr
    assert r.returncode == 0, text[-4000:]
    agg = json.loads(re.search(r"MDT_AGGREGATE (.*)", text).group(1))
    assert agg["failed_trials"] == [] and agg["binarize"] == "dynamic" and agg["samples"] == 1024
    assert np.isfinite(agg["iw_nll"]["0"])
    assert re.search(r"^\[0:0\] ====> Test set IW-5 NLL: \d+\.\d{4} ELBO-5: \d+\.\d{4}$", text, re.M)
    rec = [json.loads(l) for l in open(tmp_path / "m" / "trial-0.jsonl")]
    ep = [x for x in rec if "epoch" in x]
    assert len(ep) == 2 and all(x["binarize_s"] > 0 for x in ep)
    assert (tmp_path / "results-0" / "reconstruction_2.png").exists()
