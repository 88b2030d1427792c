"""``run_trial`` and ``run_packed_trials`` on one trial give the same result
(torch backend, MLP): they share the resume, data-binding and after-trial
helpers of hpo/runner.py."""
import math

from tests import lifecycle_cases as lc


def test_single_and_packed_paths_agree_on_one_trial(tmp_path, capsys):
    # Measured on the code before the shared helpers: no field differs between the two paths
    # beyond the timings set aside by ``lifecycle_cases._timeless`` and the "(trial 0) " tag of
    # the packed path's stdout lines.
    r = lc.run_both("mlp", "torch", tmp_path)
    a, b = r["single"], r["packed"]
    for x in (a, b):
        res = x["result"]
        assert not res.failed, res.error
        assert (res.epochs, res.shard, res.samples) == (1, lc.N_TRAIN, lc.N_TRAIN)
        assert set(x["extra"]) == {"iw_nll", "iw_neg_elbo", "iw_samples", "latent", "test_loss_raw"}
        assert all(math.isfinite(x["extra"][k]) for k in ("iw_nll", "iw_neg_elbo", "test_loss_raw"))
        assert x["extra"]["latent"]["free_bits"] == 0.05 and "below_floor" in x["extra"]["latent"]
    assert a["extra"] == b["extra"]
    assert a["result"].final_train_loss == b["result"].final_train_loss
    assert a["result"].final_test_loss == b["result"].final_test_loss
    assert a["result"].extra["test_loss_raw"] != a["result"].final_test_loss   # raw weights against averaged ones
    # metrics: an epoch record with the knob fields in the table's order, then the two passes' events
    assert a["events"] == b["events"] and [list(e) for e in a["events"]] == [list(e) for e in b["events"]]
    epoch = a["events"][0]
    knob_keys = [k for k in epoch if k in ("free_bits", "train_tc", "tc_weight", "ema_decay")]
    assert knob_keys == ["free_bits", "train_tc", "tc_weight", "ema_decay"] and epoch["ema_decay"] == 0.9
    assert [e.get("event") for e in a["events"]] == [None, "iw_eval", "latent_eval"]
    # checkpoints: the same keys, equal tensors, and the record of all three knobs
    assert lc.same_nested(a["ckpt"], b["ckpt"])
    assert a["ckpt"]["objective"] == lc.KNOBS and "ema" in a["ckpt"]["optimizer"]
    out = capsys.readouterr().out
    assert "====> Test set IW-2 NLL" in out and "(trial 0) ====> Test set IW-2 NLL" in out
