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
PRDC_KEYS = ("k", "precision", "recall", "density", "coverage")
SWD_KEYS = ("dirs", "swd1", "swd1_se", "swd2", "max_w1")
SINKHORN_KEYS = ("blur", "iters", "scale", "sinkhorn", "w2", "ot", "marg_err")
NDB_KEYS = ("K", "iters", "ndb", "ndb_over_k", "jsd", "missing", "inertia", "moved")
GMM_KEYS = ("k", "iters", "rows_fit", "ll_fit", "ll_test", "lp_test", "gap", "min_weight")
RECON_KEYS = ("mse", "psnr", "ssim", "ssim_l", "ssim_cs", "ssim_min")


def trial_record(result, opts) -> dict:
    """One rank's record of one trial it took part in."""
    rec = dict(group_id=result.group_id, samples=result.samples, wall_s=result.wall_s, failed=result.failed,
               **{k: result.extra.get(k) for k in SCORES})
    if opts.sample_report > 0:  # only then: the default record stays what it was
        rec["sample_report"] = result.extra.get("sample_report")
    if opts.prdc_k > 0:
        rec["prdc"] = result.extra.get("prdc")
    if opts.recon_report:
        rec["recon_report"] = result.extra.get("recon_report")
    if opts.swd_dirs > 0:
        rec["swd"] = result.extra.get("swd")
    if opts.gmm_k > 0:
        rec["gmm"] = result.extra.get("gmm")
    if opts.sinkhorn_blur > 0:
        rec["sinkhorn"] = result.extra.get("sinkhorn")
    if opts.ndb_k > 0:
        rec["ndb"] = result.extra.get("ndb")
    return rec


def summarize(gathered, specs, opts) -> dict:
    """``gathered``: per rank, the list of its ``trial_record``s (None or empty: an idle rank)."""
    per_trial, wall, failed = {}, 0.0, set()
    scores = {k: {} for k in SCORES + ("sample_report", "prdc", "recon_report", "swd", "gmm", "sinkhorn", "ndb")}
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
    if opts.prdc_k > 0:
        # fidelity (precision, density) and diversity (recall, coverage) on k-NN radii: four numbers, no single order
        summary["prdc"] = {str(g): {k: (v[k] if k == "k" else round(v[k], 6)) for k in PRDC_KEYS}
                           for g, v in sorted(scores["prdc"].items())}
    if opts.recon_report:
        # test images against their reconstructions from the posterior mean: the largest mean SSIM is the best trial
        recon = scores["recon_report"]
        summary["recon_report"] = {str(g): {k: round(v[k], 6) for k in RECON_KEYS} for g, v in sorted(recon.items())}
        summary["best_trial_by_ssim"] = (min(recon, key=lambda g: (-recon[g]["ssim"], g)) if recon else None)
    if opts.swd_dirs > 0:
        # a distance in the units of the data with its Monte-Carlo error over the directions: the lowest is the best trial
        w = scores["swd"]
        summary["swd"] = {str(g): {k: (v[k] if k == "dirs" else round(v[k], 6)) for k in SWD_KEYS} for g, v in sorted(w.items())}
        summary["best_trial_by_swd"] = min(w, key=lambda g: (w[g]["swd1"], g)) if w else None
    if opts.gmm_k > 0:
        # samples of the fitted mixture against the same test rows: the order by MMD with the prior hole taken out
        m = scores["gmm"]
        summary["gmm"] = {str(g): dict({k: (v[k] if k in ("k", "iters", "rows_fit") else round(v[k], 6)) for k in GMM_KEYS},
                                       **{k: round(v["sample_report"][k], 6) for k in SAMPLE_KEYS})
                          for g, v in sorted(m.items())}
        summary["best_trial_by_gmm_mmd2"] = min(m, key=lambda g: (m[g]["sample_report"]["mmd2"], g)) if m else None
    if opts.sinkhorn_blur > 0:
        # the debiased entropic transport distance in the squared units of the data: the lowest is the best trial
        w = scores["sinkhorn"]
        summary["sinkhorn"] = {str(g): {k: (v[k] if k in ("blur", "iters") else float(f"{v[k]:.6g}")) for k in SINKHORN_KEYS}
                               for g, v in sorted(w.items())}
        summary["best_trial_by_sinkhorn"] = min(w, key=lambda g: (w[g]["sinkhorn"], g)) if w else None
    if opts.ndb_k > 0:
        # mode coverage on k-means bins of the test rows: the lowest divergence of the two histograms is the best trial
        w = scores["ndb"]
        summary["ndb"] = {str(g): {k: (float(f"{v[k]:.6g}") if k in ("ndb_over_k", "jsd", "inertia") else v[k]) for k in NDB_KEYS}
                          for g, v in sorted(w.items())}
        summary["best_trial_by_ndb_jsd"] = min(w, key=lambda g: (w[g]["jsd"], g)) if w else None
    return summary
