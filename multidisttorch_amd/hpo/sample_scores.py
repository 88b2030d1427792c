"""The scores of a trial's after-trial reports: one row each, read by everything above the kernels.

``SCORES`` holds the scores that ride on the sample pass (``--sample-report N``):
a row's key is its name in the ``evaluate_samples`` result, in ``TrialResult.extra``,
in the trial record and in the summary. vae-hpo.py, hpo/runner.py and
hpo/aggregate.py loop over it; ``SampleEval`` (models/eval_graphs.py) keeps one
compute function per key. ``REPORTS`` adds the passes with code paths of their own
(the sample pass itself, the mixture pass that embeds the others, the recon pass)
in the order the trial record and the summary list them; of those only the record
and summary columns are used. docs/SAMPLE_SCORES.md lists what a new row leaves to
do. This module imports nothing of the package; a row's domain check is imported
where it is called.
"""

from __future__ import annotations

import importlib
from dataclasses import dataclass

RAW, R6, G6 = "raw", "round6", "6g"  # a summary value: as it is, round(v, 6), float(f"{v:.6g}")
_RULES = {RAW: lambda v: v, R6: lambda v: round(v, 6), G6: lambda v: float(f"{v:.6g}")}


@dataclass(frozen=True)
class Flag:
    name: str      # on the command line
    type: type
    default: object
    metavar: str
    help: str
    field: str     # of RunOptions
    kwarg: str     # of evaluate_samples

    @property
    def dest(self) -> str:
        return self.name[2:].replace("-", "_")


@dataclass(frozen=True)
class Score:
    key: str
    field: str                # the RunOptions field that turns it on (> 0)
    summary: tuple            # ((key or dotted path into the result, rule), ...): the summary entry's keys, in order
    best: tuple = None        # (summary key, result key or path, +1 lowest / -1 highest is best); ties: the lower group id
    header: tuple = None      # (summary key, RunOptions field) written before the entry
    # ---- the rows of SCORES only ----
    flags: tuple = ()         # the main flag, then its -iters flag
    check: tuple = None       # (module under models, function): called with (N, N, 1, *flag values) at parse time
    needs: str = ""           # the refusal without --sample-report
    line: str = ""            # the stdout line after "====> Test set ", and the result keys it formats
    line_keys: tuple = ()
    group_kwarg: str = None   # the evaluate_samples keyword that takes the trial's group id

    def kwargs(self, opts, metrics) -> dict:
        """The ``evaluate_samples`` keywords of this score, none when it is off: the default call stays the call it
        was. ``metrics``: the trial's, read for its ``group_id`` by a score that takes one."""
        if not getattr(opts, self.field) > 0:
            return {}
        kw = {f.kwarg: f.type(getattr(opts, f.field)) for f in self.flags}
        if self.group_kwarg:
            kw[self.group_kwarg] = int(metrics.group_id)
        return kw

    def check_args(self, args):
        """At parse time: ValueError when the flags are set without ``--sample-report`` or outside the domain."""
        main = self.flags[0]
        if getattr(args, main.dest) == 0:
            return
        fn = getattr(importlib.import_module("multidisttorch_amd.models." + self.check[0]), self.check[1])
        if args.sample_report == 0:
            raise ValueError(self.needs)
        fn(args.sample_report, args.sample_report, 1, *[getattr(args, f.dest) for f in self.flags])

    def format(self, result: dict) -> str:
        return self.line.format(*[result[k] for k in self.line_keys])

    def summarize(self, per_trial: dict, summary: dict, opts):
        """``per_trial``: group id -> this score's result. Adds the header, the entry and the best trial to ``summary``."""
        if self.header:
            summary[self.header[0]] = getattr(opts, self.header[1])
        summary[self.key] = {str(g): {path.rsplit(".", 1)[-1]: _RULES[rule](_get(v, path)) for path, rule in self.summary}
                             for g, v in sorted(per_trial.items())}
        if self.best:
            name, path, sign = self.best
            summary[name] = min(per_trial, key=lambda g: (sign * _get(per_trial[g], path), g)) if per_trial else None


def _get(v: dict, path: str):
    for k in path.split("."):
        v = v[k]
    return v


def _cols(rule, *keys):
    return tuple((k, rule) for k in keys)


SCORES = (
    # fidelity (precision, density) and diversity (recall, coverage) on k-NN radii: four numbers, no single order
    Score("prdc", "prdc_k", _cols(RAW, "k") + _cols(R6, "precision", "recall", "density", "coverage"),
          flags=(Flag("--prdc", int, 0, "K",
                      "with --sample-report N: also precision, recall, density and coverage of the same rows "
                      "on K-nearest-neighbour radii (fidelity against diversity; 1 <= K <= 8 < N; 0 = off)",
                      "prdc_k", "prdc_k"),),
          check=("prdc", "check_prdc_args"),
          needs="--prdc K scores the rows of the sample pass: it needs --sample-report N",
          line="PRDC-{}: precision {:.4f} recall {:.4f} density {:.4f} coverage {:.4f}",
          line_keys=("k", "precision", "recall", "density", "coverage")),
    # a distance in the units of the data with its Monte-Carlo error over the directions: the lowest is the best trial
    Score("swd", "swd_dirs", _cols(RAW, "dirs") + _cols(R6, "swd1", "swd1_se", "swd2", "max_w1"),
          best=("best_trial_by_swd", "swd1", 1),
          flags=(Flag("--swd", int, 0, "P",
                      "with --sample-report N: also the sliced Wasserstein distance of the same rows over P "
                      "random unit directions, with its standard error (a distance in the units of the data; "
                      "2 <= N <= 16384, 1 <= P <= 4096; 0 = off)",
                      "swd_dirs", "swd_dirs"),),
          check=("swd", "check_swd_args"),
          needs="--swd P scores the rows of the sample pass: it needs --sample-report N",
          line="SWD-{}: W1 {:.6f} +- {:.6f} W2 {:.6f} max {:.6f}",
          line_keys=("dirs", "swd1", "swd1_se", "swd2", "max_w1")),
    # the debiased entropic transport distance in the squared units of the data: the lowest is the best trial
    Score("sinkhorn", "sinkhorn_blur", _cols(RAW, "blur", "iters") + _cols(G6, "scale", "sinkhorn", "w2", "ot", "marg_err"),
          best=("best_trial_by_sinkhorn", "sinkhorn", 1),
          flags=(Flag("--sinkhorn", float, 0.0, "E",
                      "with --sample-report N: also the Sinkhorn divergence (debiased entropic optimal transport) "
                      "of the same rows at blur E, a fraction of the test rows' mean squared distance: a "
                      "full-dimensional transport distance in the squared units of the data "
                      "(2 <= N <= 16384, 0 < E <= 4; 0 = off)",
                      "sinkhorn_blur", "sinkhorn_blur"),
                 Flag("--sinkhorn-iters", int, 100, "T",
                      "annealed iterations of --sinkhorn (a fixed count, 1 <= T <= 10000)",
                      "sinkhorn_iters", "sinkhorn_iters")),
          check=("sinkhorn", "check_sinkhorn_args"),
          needs="--sinkhorn E scores the rows of the sample pass: it needs --sample-report N",
          line="Sinkhorn-{:g}: S {:.6f} W2 {:.6f} OT {:.6f} marg err {:.3e} ({} iters)",
          line_keys=("blur", "sinkhorn", "w2", "ot", "marg_err", "iters")),
    # mode coverage on k-means bins of the test rows: the lowest divergence of the two histograms is the best trial
    Score("ndb", "ndb_k", (("K", RAW), ("iters", RAW), ("ndb", RAW), ("ndb_over_k", G6), ("jsd", G6), ("missing", RAW),
                           ("inertia", G6), ("moved", RAW)),
          best=("best_trial_by_ndb_jsd", "jsd", 1),
          flags=(Flag("--ndb", int, 0, "K",
                      "with --sample-report N: also which kinds of image are missing: the N test rows are "
                      "clustered into K k-means bins in pixel space, and the number of bins whose real and "
                      "generated shares differ significantly (NDB), the Jensen-Shannon divergence of the two "
                      "histograms and the bins without a generated row are reported (2 <= K <= 256, K <= N; 0 = off)",
                      "ndb_k", "ndb"),
                 Flag("--ndb-iters", int, 20, "T",
                      "Lloyd iterations of the --ndb bins (a fixed count, 1 <= T <= 1000)",
                      "ndb_iters", "ndb_iters")),
          check=("ndb", "check_ndb_args"),
          needs="--ndb K bins the rows of the sample pass: it needs --sample-report N",
          line="NDB-{}: ndb {} ({:.3f}) JSD {:.4f} missing {} inertia {:.6g} moved {} ({} iters)",
          line_keys=("K", "ndb", "ndb_over_k", "jsd", "missing", "inertia", "moved", "iters"),
          # the starting rows of the bins come from the run seed and the trial: both backends see the same indices
          group_kwarg="ndb_group"),
)
BY_KEY = {s.key: s for s in SCORES}
KEYS = tuple(BY_KEY)
FIELDS = tuple(f.field for s in SCORES for f in s.flags)  # of RunOptions, with the flags' defaults

_SAMPLE_COLS = ("mmd2", "nn_acc", "nn_acc_real", "nn_acc_fake")
# the trial record and the summary, in this order
REPORTS = (
    # prior samples against test rows: the lowest kernel MMD is the best trial; 1-NN accuracy 0.5 is ideal
    Score("sample_report", "sample_report", _cols(R6, *_SAMPLE_COLS), best=("best_trial_by_mmd2", "mmd2", 1),
          header=("sample_rows", "sample_report")),
    BY_KEY["prdc"],
    # test images against their reconstructions from the posterior mean: the largest mean SSIM is the best trial
    Score("recon_report", "recon_report", _cols(R6, "mse", "psnr", "ssim", "ssim_l", "ssim_cs", "ssim_min"),
          best=("best_trial_by_ssim", "ssim", -1)),
    BY_KEY["swd"],
    # samples of the fitted mixture against the same test rows: the order by MMD with the prior hole taken out
    Score("gmm", "gmm_k", _cols(RAW, "k", "iters", "rows_fit") + _cols(R6, "ll_fit", "ll_test", "lp_test", "gap", "min_weight")
          + _cols(R6, *("sample_report." + k for k in _SAMPLE_COLS)),
          best=("best_trial_by_gmm_mmd2", "sample_report.mmd2", 1)),
    BY_KEY["sinkhorn"],
    BY_KEY["ndb"],
)
