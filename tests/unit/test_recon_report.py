"""The reconstruction report (models/recon_report.py) on the CPU: the oracle
against the definition written out window by window, three identities, the
domain, the flag, the aggregate's keys and one torch-backend runner pass."""
import importlib.util
import math
import os
import types

import pytest
import torch

from multidisttorch_amd.hpo import runner
from multidisttorch_amd.hpo.aggregate import summarize, trial_record
from multidisttorch_amd.hpo.trial import build_specs
from multidisttorch_amd.models import recon_report as rr
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer
from tests import recon_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _direct_rows(real, recon, S):
    """The definition in Python floats: every window, every one of its 121 terms."""
    g = [math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)]
    tot = sum(a * b for a in g for b in g)
    rows = []
    for x, r in zip(real.reshape(-1, S, S).tolist(), recon.reshape(-1, S, S).tolist()):
        acc = [0.0, 0.0, 0.0]
        for i in range(S - 10):
            for j in range(S - 10):
                win = [(g[a] * g[b] / tot, x[i + a][j + b], r[i + a][j + b]) for a in range(11) for b in range(11)]
                mx, my = sum(w * p for w, p, _ in win), sum(w * q for w, _, q in win)
                vx, vy = sum(w * p * p for w, p, _ in win) - mx * mx, sum(w * q * q for w, _, q in win) - my * my
                vxy = sum(w * p * q for w, p, q in win) - mx * my
                l, cs = (2 * mx * my + rr.C1) / (mx * mx + my * my + rr.C1), (2 * vxy + rr.C2) / (vx + vy + rr.C2)
                acc = [acc[0] + l * cs, acc[1] + l, acc[2] + cs]
        se = sum((p - q) ** 2 for xr, rr_ in zip(x, r) for p, q in zip(xr, rr_))
        rows.append([se] + [a / (S - 10) ** 2 for a in acc])
    return torch.tensor(rows, dtype=torch.float64)


@pytest.mark.parametrize("S", [11, 12, 14])
@pytest.mark.parametrize("family", ["random", "edge"])
def test_oracle_is_the_definition(family, S):
    real, recon = (t.double() for t in rc.FAMILIES[family](3, S))
    assert torch.allclose(rr.recon_rows(real, recon, S), _direct_rows(real, recon, S), rtol=1e-12, atol=1e-13)


def test_identities():
    x, _ = rc.random(4, 16)
    x = x.double()
    same = rr.recon_rows(x, x.clone(), 16)
    assert torch.equal(same[:, 0], torch.zeros(4, dtype=torch.float64))
    assert torch.allclose(same[:, 1:], torch.ones(4, 3, dtype=torch.float64), rtol=0, atol=1e-13)
    assert bool((rr.recon_rows(x, 1 - x, 16)[:, 3] < 0).all())        # the negative: anti-correlated structure
    base, dim = rr.recon_rows(0.5 * x, 0.45 * x + 0.05, 16), rr.recon_rows(0.5 * x + 0.3, 0.45 * x + 0.35, 16)
    assert torch.allclose(dim[:, 3], base[:, 3], rtol=1e-12, atol=0)  # brightness + 0.3 on both: cs stays,
    assert bool(((dim[:, 2] - base[:, 2]).abs() > 1e-3).all())        # l moves
    s = rr.recon_stats(torch.tensor([[0.0, 1.0, 1.0, 1.0], [8.0, 0.5, 0.75, 0.25]]), 16)
    assert s == dict(rows=2, side=16, mse=1 / 64, psnr=-10 * math.log10(1 / 64), ssim=0.75, ssim_l=0.875, ssim_cs=0.625,
                     ssim_min=0.5)


@pytest.mark.parametrize("n,D", [(0, 784), ((1 << 20) + 1, 784), (4, 100), (4, 785), (4, 257 ** 2), (4, 0)])
def test_domain(n, D):
    with pytest.raises(ValueError, match="reconstruction report supports"):
        rr.check_recon_args(n, D)
    assert rr.check_recon_args(1, 121) == 11 and rr.check_recon_args(1 << 20, 65536) == 256 and rr.COLS == 4


def test_flag_reaches_the_options_and_the_aggregate():
    spec = importlib.util.spec_from_file_location("vae_hpo_cli_recon", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args([]).recon_report is False and mod.parse_args(["--recon-report"]).recon_report is True
    off, on = runner.RunOptions(), runner.RunOptions(recon_report=True)
    row = [r for r in runner._AFTER_TRIAL if r[2] is runner._recon_eval][0]
    assert not row[1](build_specs(1, 1)[0], off) and row[1](build_specs(1, 1)[0], on)
    with pytest.raises(ValueError, match="got D = 20"):   # at run start, before any training
        runner._check_recon_data(on, _Test(torch.zeros(8, 20)))
    runner._check_recon_data(off, _Test(torch.zeros(8, 20)))
    rep = lambda ssim: dict(mse=0.0123456789, psnr=19.0848, ssim=ssim, ssim_l=0.9, ssim_cs=0.8, ssim_min=0.1)
    res = [runner.TrialResult(g, 2, 128, 256, 1.5, 0.1, 0.2, extra=dict(recon_report=rep(s)))
           for g, s in ((0, 0.5), (1, 0.75), (2, 0.75))]
    assert all("recon_report" not in trial_record(r, off) for r in res)
    s_off, s_on = (summarize([[trial_record(r, o) for r in res]], build_specs(3, 1), o) for o in (off, on))
    assert list(s_on) == list(s_off) + ["recon_report", "best_trial_by_ssim"] and s_on["best_trial_by_ssim"] == 1
    assert s_on["recon_report"]["0"] == dict(rep(0.5), mse=0.012346)


class _Test:
    def __init__(self, X):
        self.data = X

    def __len__(self):
        return self.data.shape[0]


def test_runner_pass_on_the_torch_backend(capsys):
    tr = MlpVaeTrainer(batch_size=16, D=144, H=20, Z=4, backend="torch", device="cpu", lr=3e-3, seed=3)
    X = torch.rand(40, 144, generator=torch.Generator().manual_seed(7))
    rows = []
    m = types.SimpleNamespace(log=lambda **kw: rows.append(kw))
    r = runner._recon_eval(tr, _Test(X), runner.RunOptions(recon_report=True), None, m, torch.device("cpu"))["recon_report"]
    assert r["rows"] == 40 and r["side"] == 12 and all(math.isfinite(v) for v in r.values())
    assert rows == [dict(event="recon_eval", **r)]
    assert capsys.readouterr().out.strip().endswith(
        "====> Test set recon: MSE {:.6f} PSNR {:.2f} SSIM {:.4f} (l {:.4f} cs {:.4f})".format(
            r["mse"], r["psnr"], r["ssim"], r["ssim_l"], r["ssim_cs"]))
    full = tr.evaluate_recon(X, torch.arange(40), return_rows=True)
    assert torch.equal(full["recon"], tr.decode(full["mu"])) and torch.equal(full["real"], X)
    assert torch.equal(full["table"], rr.recon_rows(X, full["recon"], 12)) and full["ssim"] == r["ssim"]
    with pytest.raises(RuntimeError, match="no evaluate_latent pass"):
        tr.latent_buffers()
