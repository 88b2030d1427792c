"""The run's summary: what every rank contributes, and what rank 0 prints as ``MDT_AGGREGATE``
and writes to ``aggregate.json`` (vae-hpo.py gathers the records in between). Aggregate
samples/s: a trial's samples count once (the minimum over its ranks), the wall
time is the maximum over all ranks."""

from __future__ import annotations

from .objective import NAMES

__all__ = ["trial_record", "summarize"]

LATENT_KEYS = ("kl", "active_units", "mi", "tc", "dwkl")
# per-trial scores of the after-trial passes (``TrialResult.extra``); None where the pass did not run
SCORES = ("iw_nll", "latent", "test_loss_raw")
SAMPLE_KEYS = ("mmd2", "nn_acc", "nn_acc_real", "nn_acc_fake")


def trial_record(result, opts) -> dict:
    """One rank's record of one trial it took part in."""
    rec = dict(group_id=result.group_id, samples=result.samples, wall_s=result.wall_s, failed=result.failed,
               **{k: result.extra.get(k) for k in SCORES})
    if opts.sample_report > 0:  # only then: the default record stays what it was
        rec["sample_report"] = result.extra.get("sample_report")
    return rec


def summarize(gathered, specs, opts) -> dict:
    """``gathered``: per rank, the list of its ``trial_record``s (None or empty: an idle rank)."""
    per_trial, wall, failed = {}, 0.0, set()
    scores = {k: {} for k in SCORES + ("sample_report",)}
    for lst in gathered:
        for r in lst or []:
            gid = r["group_id"]
            per_trial[gid] = min(per_trial.get(gid, r["samples"]), r["samples"])
            wall = max(wall, r["wall_s"])
            if r["failed"]:
                failed.add(gid)
            for k in scores:
                if r.get(k) is not None:
                    scores[k][gid] = r[k]
    iw_nll, latent = scores["iw_nll"], scores["latent"]
    summary = {"metric": "aggregate VAE samples/sec across K concurrent HPO trials",
               "trials": len(per_trial), "samples": int(sum(per_trial.values())),
               "wall_s": round(wall, 4),
               "value": round(sum(per_trial.values()) / max(wall, 1e-9), 1), "unit": "samples/s",
               "failed_trials": sorted(failed)}
    if opts.binarize != "none":
        summary["binarize"] = opts.binarize  # the likelihood every score of this run is under
    for name in NAMES:
        if name in opts.report_objective:
            # every trial's value of a knob of the training objective; test scores are the true ELBO terms
            summary[name] = {str(s.group_id): getattr(s, name) for s in specs}
            if name == "ema_decay":
                # every score of a trial that sets a decay is under the averaged weights, and test_loss_raw
                # is its last test loss under the raw ones (what averaging bought)
                summary["test_loss_raw"] = {str(g): round(v, 4) for g, v in sorted(scores["test_loss_raw"].items())}
    if opts.iw_samples > 0:
        # per-image means over the test set; the lowest bound on -log p(x) is the best trial
        summary["iw_samples"] = opts.iw_samples
        summary["iw_nll"] = {str(g): round(v, 4) for g, v in sorted(iw_nll.items())}
        summary["best_trial_by_iw_nll"] = min(iw_nll, key=lambda g: (iw_nll[g], g)) if iw_nll else None
    if opts.latent_report:
        # per-image means over the test set (nats); active_units counts Var_x(mu_d) > --au-threshold
        summary["latent"] = {str(g): {k: (v[k] if k == "active_units" else round(v[k], 4)) for k in LATENT_KEYS}
                             for g, v in sorted(latent.items())}
        for g, v in latent.items():  # trials with a KL floor: the dimensions it holds up
            if "below_floor" in v:
                summary["latent"][str(g)]["below_floor"] = v["below_floor"]
    if opts.sample_report > 0:
        # prior samples against test rows: the lowest kernel MMD is the best trial; 1-NN accuracy 0.5 is ideal
        samples = scores["sample_report"]
        summary["sample_rows"] = opts.sample_report
        summary["sample_report"] = {str(g): {k: round(v[k], 6) for k in SAMPLE_KEYS} for g, v in sorted(samples.items())}
        summary["best_trial_by_mmd2"] = (min(samples, key=lambda g: (samples[g]["mmd2"], g)) if samples else None)
    return summary
