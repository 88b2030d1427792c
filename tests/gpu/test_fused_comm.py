"""Fused xGMI all-reduce jobs in the conv-VAE step (csrc/kernels/comm_jobs.h).

The reference's intra-group DDP (/root/reference/vae-hpo.py:72, :130) launches
bucket all-reduces from autograd hooks on NCCL's stream and runs foreach-Adam
after the wait. Here, with a fused XgmiP2PReducer ("xgmi"), the all-reduce is
a set of JOBS inside the step's own launches (models/conv28.py::_step28; the
layer path: models/conv_layers.py::_comm_tail): the decoder units' push runs in
the launch that computes the encoder weight gradients, and one tail launch
does push+reduce (encoder) || reduce (decoder) with Adam fused in.

On a group of ONE rank the jobs still run (finalize -> scale -> Adam), so the
DDP step structure is exercised and timed on a one-GPU box:
  * scale 1: results are BITWISE the reducer-free step (same slab summation
    helpers, x * 1.0, same Adam arithmetic), pair kernel on and off, eager and
    graph-replayed, overlap and no-overlap schedules;
  * scale 2 with Adam's grad_scale 0.5: bitwise too (exact powers of two),
    which proves the scaled reduce actually ran on every unit;
  * the DDP step costs at most ~1.15x the reducer-free step (the verdict's
    structure-cost bar; measured numbers in profiles/r4_ddp_fused).

The values with MORE than one rank (different gradients per rank) are checked
in tests/gpu/test_comm_jobs_values.py.
"""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _data(nb, B, dev):
    X = torch.rand(nb * B, 784, generator=torch.Generator().manual_seed(3)).to(dev)
    return X, torch.arange(nb * B, device=dev, dtype=torch.int32)


def _trainer(dev, graphs, pair=True, overlap=True, graph_steps=4):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    tr = ConvVaeTrainer(batch_size=128, image=28, z=32, device=dev, backend="hip", seed=4, lr=2e-3,
                        use_graphs=graphs, graph_steps=graph_steps)
    assert tr.f28
    tr.f28_pair = pair
    tr.ddp_overlap = overlap
    return tr


def _fused_reducer(tr, scale=0.0):
    C = tr.C
    red = C.XgmiP2PReducer(0, 1, tr.grads, tr.default_bucket_bounds(), True, float(scale), 64, 20.0, -1, True)
    assert red.fused()
    return red


def _run(tr, X, idx, nb, steps):
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, nb)
    tr.train_steps(steps)
    torch.cuda.synchronize()
    return tr.params.clone(), tr.loss_history()[:steps].copy()


def _explain(make_ref, nb, steps, X, idx, p1, h1, p0, h0, layer_ranges):
    """On a mismatch: which side moves (the reference re-run twice) and in
    which layers the parameters differ -- printed for the log."""
    if torch.equal(p1, p0) and (h1 == h0).all():
        return
    reruns = [_run(make_ref(), X, idx, nb, steps) for _ in range(2)]
    same_ref = [bool(torch.equal(p, p0)) for p, _ in reruns]
    same_fused = [bool(torch.equal(p, p1)) for p, _ in reruns]
    diff = {l.name: float((p1[b:e] - p0[b:e]).abs().max()) for l, b, e in layer_ranges}
    first = int(np.argmax(h1 != h0)) if (h1 != h0).any() else -1
    print(f"MISMATCH first differing loss step {first}; reference re-runs equal to the first reference "
          f"{same_ref}, equal to the fused run {same_fused}; per-layer max |dp| {diff}", flush=True)


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("pair", [True, False])
@pytest.mark.parametrize("overlap", [True, False])
def test_fused_reducer_one_rank_is_bitwise_reducer_free(native_ext, graphs, pair, overlap):
    dev = torch.device("cuda", 0)
    nb, steps = 4, 8
    X, idx = _data(nb, 128, dev)
    p0, h0 = _run(_trainer(dev, graphs, pair, overlap), X, idx, nb, steps)
    tr = _trainer(dev, graphs, pair, overlap)
    red = _fused_reducer(tr)
    tr.attach_reducer(red)
    p1, h1 = _run(tr, X, idx, nb, steps)
    assert int(red.status()) == 0
    assert int(tr.f28_err.item()) == 0
    assert red.launched_count() == 0  # no stream-side collectives: everything ran as jobs
    assert np.isfinite(h0).all() and tr.read_state()["step"] == steps
    _explain(lambda: _trainer(dev, graphs, pair, overlap), nb, steps, X, idx, p1, h1, p0, h0, tr.layer_ranges())
    np.testing.assert_array_equal(h1, h0)
    assert torch.equal(p1, p0), (p1 - p0).abs().max().item()


@pytest.mark.parametrize("overlap", [True, False])
def test_fused_reducer_scaled_reduce_runs_on_every_unit(native_ext, overlap):
    """scale 2 in the reduce, grad_scale 0.5 in Adam: equal to the plain step
    only if every unit's reduce ran (a skipped unit keeps the unscaled
    gradient and its parameters drift by Adam's 1/sqrt scaling)."""
    dev = torch.device("cuda", 0)
    nb, steps = 4, 8
    X, idx = _data(nb, 128, dev)
    p0, h0 = _run(_trainer(dev, True, overlap=overlap), X, idx, nb, steps)
    tr = _trainer(dev, True, overlap=overlap)
    tr.attach_reducer(_fused_reducer(tr, scale=2.0))
    tr.set_hparams(grad_scale=0.5)
    p1, h1 = _run(tr, X, idx, nb, steps)
    _explain(lambda: _trainer(dev, True, overlap=overlap), nb, steps, X, idx, p1, h1, p0, h0, tr.layer_ranges())
    np.testing.assert_array_equal(h1, h0)
    assert torch.equal(p1, p0), (p1 - p0).abs().max().item()


def test_fused_reducer_skip_adam_leaves_reduced_grads(native_ext):
    """f28_skip_adam: the tail writes the scaled, reduced gradient into the
    arena instead of applying Adam; equal to the reducer-free finalize x scale."""
    dev = torch.device("cuda", 0)
    X, idx = _data(2, 128, dev)
    ref = _trainer(dev, False)
    ref.f28_skip_adam = True
    ref.bind_train_data(X, idx)
    ref.set_cursor(0, 2)
    ref.train_steps(1)
    tr = _trainer(dev, False)
    tr.f28_skip_adam = True
    tr.attach_reducer(_fused_reducer(tr, scale=2.0))
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, 2)
    tr.train_steps(1)
    torch.cuda.synchronize()
    assert torch.equal(tr.grads, 2.0 * ref.grads)
    assert torch.equal(tr.params, ref.params)  # no update


def _time_steps(tr, X, idx, nb, reps=5, steps=20):
    tr.graph_steps = steps
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, nb)
    tr.prepare([128])
    tr.train_steps(steps)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        tr.train_steps(steps)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / steps)
    return best * 1e6


def test_fused_ddp_step_cost_vs_reducer_free(native_ext):
    """Structure cost of intra-group DDP on the headline step: one-rank fused
    reducer (all jobs run, nothing to move) vs no reducer, 20-step graphs."""
    dev = torch.device("cuda", 0)
    nb = 8
    X, idx = _data(nb, 128, dev)
    base = _time_steps(_trainer(dev, True), X, idx, nb)
    tr = _trainer(dev, True)
    tr.attach_reducer(_fused_reducer(tr))
    ddp = _time_steps(tr, X, idx, nb)
    print(f"\nreducer-free {base:.1f} us/step, fused one-rank DDP {ddp:.1f} us/step, ratio {ddp / base:.3f}")
    assert ddp <= 1.2 * base, (base, ddp)


@pytest.mark.parametrize("image", [128, 28])
def test_fused_reducer_layer_path_bitwise(native_ext, image):
    """The layer-by-layer step (128x128; 28x28 with MDT_CONV_F28=0) with the
    fused reducer on one rank: pushes ride in the backward launches, the tail
    reduces + applies Adam; bitwise the reducer-free step, eager and graphs."""
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    dev = torch.device("cuda", 0)
    B = 32 if image == 128 else 128
    nb, steps = 4, 6
    X = torch.rand(nb * B, image * image, generator=torch.Generator().manual_seed(5)).to(dev)
    idx = torch.arange(nb * B, device=dev, dtype=torch.int32)
    for graphs in (False, True):
        out = []
        for fused in (False, True):
            tr = ConvVaeTrainer(batch_size=B, image=image, z=32 if image == 28 else 64, device=dev, backend="hip",
                                seed=6, lr=2e-3, use_graphs=graphs, graph_steps=3)
            tr.f28 = False
            if fused:
                red = _fused_reducer(tr)
                tr.attach_reducer(red)
            tr.bind_train_data(X, idx)
            tr.set_cursor(0, nb)
            tr.train_steps(steps)
            tr._ensure_wt()  # the reducer-free 28x28 layer path defers the last step's transposes
            torch.cuda.synchronize()
            out.append((tr.loss_history()[:steps].copy(), tr.params.clone(), tr.w16t.clone()))
            if fused:
                assert int(red.status()) == 0 and red.launched_count() == 0
                assert tr._fused_launches > 0
        np.testing.assert_array_equal(out[1][0], out[0][0])
        assert torch.equal(out[1][1], out[0][1]), (out[1][1] - out[0][1]).abs().max().item()
        assert torch.equal(out[1][2], out[0][2])  # transposed copies of the updated weights


def test_fused_reducer_epoch_rebase_and_abort_word(native_ext):
    """Host-side controls of the fused reducer: moving the trainer's step
    counter backwards rebases the jobs' epoch (step + base stays increasing);
    the abort word is visible to the host and a one-rank step (no waits) still
    runs bitwise after it; the uncached regions are pooled per size class."""
    dev = torch.device("cuda", 0)
    nb = 4
    X, idx = _data(nb, 128, dev)
    tr = _trainer(dev, False)
    red = _fused_reducer(tr)
    tr.attach_reducer(red)
    tr.bind_train_data(X, idx)
    tr.set_cursor(0, nb)
    tr.train_steps(3)
    torch.cuda.synchronize()
    assert red.epoch_base() == 0
    tr.set_step(10)  # forward (resume): no rebase needed
    assert red.epoch_base() == 0
    tr.set_step(2)  # backwards: base grows past the epochs already used
    assert red.epoch_base() == (10 - 2) + 2
    tr.train_steps(2)
    torch.cuda.synchronize()
    assert int(red.status()) == 0 and tr.read_state()["step"] == 4
    assert not red.aborted()
    red.abort()
    assert red.aborted()
    tr.train_steps(1)  # s = 1: nothing to wait for, the step is unaffected
    torch.cuda.synchronize()
    assert int(red.status()) == 0
    sz = red.alloc_bytes()
    assert sz >= red.region_bytes() and sz & (sz - 1) == 0  # power-of-two size class
