"""Every row of the objective-knob table (hpo/objective.py) through every place
that loops over it: the command line, ``build_specs``, the trainers' ``hp`` and
``set_hparams``, the checkpoint's ``objective`` record and the runner's resume
check. The expected error texts are written out here as the code before the
table produced them."""
import importlib.util
import os
import re

import pytest
import torch

from multidisttorch_amd.ckpt import checkpoint as ckpt
from multidisttorch_amd.hpo import objective, runner
from multidisttorch_amd.hpo.trial import TrialSpec, build_specs
from multidisttorch_amd.models.mlp_trainer import MlpVaeTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (flag, two admissible values, {bad value: the ValueError text}, recorded in a checkpoint at 0, structural)
ROWS = {
    "free_bits": ("--free-bits", (0.05, 0.25),
                  {-1.0: "free_bits must be finite and >= 0, got -1.0",
                   float("nan"): "free_bits must be finite and >= 0, got nan",
                   float("inf"): "free_bits must be finite and >= 0, got inf"}, True, False),
    "tc_weight": ("--tc-weight", (0.5, 2.0),
                  {-0.5: "tc_weight must be finite and >= 0, got -0.5",
                   float("nan"): "tc_weight must be finite and >= 0, got nan",
                   float("inf"): "tc_weight must be finite and >= 0, got inf"}, False, True),
    "ema_decay": ("--ema-decay", (0.9, 0.99),
                  {1.0: "ema_decay must be in [0, 1), got 1.0",
                   1.5: "ema_decay must be in [0, 1), got 1.5",
                   -0.1: "ema_decay must be in [0, 1), got -0.1",
                   float("nan"): "ema_decay must be in [0, 1), got nan"}, False, True),
}
NAMES = list(ROWS)


def test_the_table_has_exactly_these_rows_in_this_order():
    assert list(objective.NAMES) == NAMES == [k.name for k in objective.KNOBS]
    assert [k.flag for k in objective.KNOBS] == [ROWS[n][0] for n in NAMES]
    assert [(k.always_saved, k.structural) for k in objective.KNOBS] == [ROWS[n][3:] for n in NAMES]
    assert [f.name for f in TrialSpec.__dataclass_fields__.values()][-3:] == NAMES


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("vae_hpo_cli", os.path.join(ROOT, "vae-hpo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mlp(**kw):
    tr = MlpVaeTrainer(batch_size=16, D=20, H=20, Z=4, backend="torch", device="cpu", seed=3, lr=3e-3, **kw)
    X = torch.rand(64, 20, generator=torch.Generator().manual_seed(7))
    tr.bind_train_data(X, torch.arange(64, dtype=torch.int32))
    tr.set_cursor(0, 4)
    return tr


@pytest.mark.parametrize("name", NAMES)
def test_flag_to_specs_scalar_and_cycled_list(cli, name):
    flag, (a, b), _, _, _ = ROWS[name]
    assert getattr(cli.parse_args([]), name) is None
    assert [getattr(s, name) for s in build_specs(3, 1)] == [0.0, 0.0, 0.0]
    args = cli.parse_args([flag, str(a)])
    assert [getattr(s, name) for s in build_specs(3, 1, **{name: getattr(args, name)})] == [a, a, a]
    args = cli.parse_args([flag, f"0,{b}"])
    specs = build_specs(3, 1, **{name: getattr(args, name)})
    assert [getattr(s, name) for s in specs] == [0.0, b, 0.0]
    assert [getattr(s, name) for s in build_specs(2, 1, **{name: [a, b]})] == [a, b]
    assert [getattr(s, name) for s in build_specs(2, 1, **{name: a})] == [a, a]
    # the others stay off, the knobs come back as one mapping, and the spec round-trips through its dict
    assert specs[1].objective() == {n: (b if n == name else 0.0) for n in NAMES}
    assert TrialSpec(**specs[1].to_dict()) == specs[1]
    assert objective.reported(specs) == (name,) and objective.reported(build_specs(2, 1)) == ()
    with pytest.raises(TypeError):
        build_specs(2, 1, not_a_knob=1.0)


@pytest.mark.parametrize("name", NAMES)
def test_out_of_range_values_raise_the_same_text_everywhere(name):
    for bad, text in ROWS[name][2].items():
        for call in (lambda: objective.check(name, bad), lambda: _mlp(**{name: bad}),
                     lambda: _mlp().set_hparams(**{name: bad})):
            with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
                call()
    # build_specs: as a scalar and inside a comma list. Before the table it named ema_decay's
    # range "finite and >= 0" for a negative or non-finite decay and "[0, 1)" from 1 up; the
    # trainers always said "[0, 1)", which is the row's one text now.
    for bad, text in ROWS[name][2].items():
        for form in (bad, f"0,{bad}"):
            with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
                build_specs(2, 1, **{name: form})


def test_the_old_validator_names_are_the_table_check():
    from multidisttorch_amd.models.tc import check_tc_weight
    from multidisttorch_amd.models.trainer_base import check_ema_decay, check_free_bits

    for name, fn in (("free_bits", check_free_bits), ("tc_weight", check_tc_weight), ("ema_decay", check_ema_decay)):
        assert fn("0.5") == 0.5 and fn(0) == 0.0
        bad, text = next(iter(ROWS[name][2].items()))
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            fn(bad)


@pytest.mark.parametrize("name", NAMES)
def test_trainer_from_the_spec_and_the_structural_rule(name):
    _, (a, b), _, _, structural = ROWS[name]
    spec = build_specs(1, 1, **{name: a})[0]
    tr = _mlp(**spec.objective())
    assert {n: tr.hp[n] for n in NAMES} == spec.objective()
    tr.set_hparams(**{name: b})
    assert tr.hp[name] == b
    tr.set_hparams(**{name: 0.0})     # built with it: turning it down to 0 is accepted
    assert tr.hp[name] == 0.0
    plain = _mlp()
    assert plain.hp[name] == 0.0
    if structural:
        text = f"{name} > 0 needs a trainer built with {name} > 0 (the step's launch list differs)"
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            plain.set_hparams(**{name: a})
        assert plain.hp[name] == 0.0
    else:
        plain.set_hparams(**{name: a})
        assert plain.hp[name] == a
    assert (tr.tc_on, tr.ema_on) == (name == "tc_weight", name == "ema_decay")
    assert (plain.tc_on, plain.ema_on) == (False, False)


@pytest.mark.parametrize("name", NAMES)
def test_checkpoint_record_and_resume_check(name, tmp_path):
    flag, (a, b), _, always, _ = ROWS[name]
    spec = build_specs(1, 2, **{name: a})[0]
    tr = _mlp(**spec.objective())
    tr.train_steps(2)
    path = ckpt.save_trial(str(tmp_path / "ck"), tr, spec, 1)
    rec = torch.load(path, weights_only=True)["objective"]
    assert rec == {"free_bits": a if name == "free_bits" else 0.0, **({} if name == "free_bits" else {name: a})}
    prog = ckpt.load_latest(str(tmp_path / "ck"), 0, _mlp(**spec.objective()))
    assert {n: prog[n] for n in NAMES} == spec.objective() and prog["binarize"] == "none"
    # a trainer without the knob: the key is there exactly when the row says "always"
    spec0 = build_specs(1, 2)[0]
    path0 = ckpt.save_trial(str(tmp_path / "ck0"), _mlp(), spec0, 1)
    assert torch.load(path0, weights_only=True)["objective"] == {"free_bits": 0.0}
    assert (name in torch.load(path0, weights_only=True)["objective"]) == always
    prog0 = ckpt.load_latest(str(tmp_path / "ck0"), 0, _mlp())
    assert all(prog0[n] == 0.0 for n in NAMES)
    # a checkpoint from before the record existed
    raw = torch.load(path0, weights_only=True)
    del raw["objective"], raw["data"]
    torch.save(raw, path0)
    old = ckpt.load_latest(str(tmp_path / "ck0"), 0, _mlp())
    assert all(old[n] == 0.0 for n in NAMES) and old["binarize"] == "none"

    opts = runner.RunOptions()
    runner._check_resumed(prog, spec, opts)      # equal values
    runner._check_resumed(None, spec, opts)      # nothing to resume from
    runner._check_resumed(old, spec0, opts)      # no record against a spec of 0
    other = build_specs(1, 2, **{name: b})[0]
    for had, want_spec, p in ((a, other, prog), (0.0, spec, old), (a, spec0, prog)):
        text = (f"trial 0: checkpoint {p['path']} was trained with {flag} {had}, "
                f"this run asks for {flag} {getattr(want_spec, name)}")
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            runner._check_resumed(p, want_spec, opts)
    was_static = dict(prog, binarize="static")
    for had, want, p in (("none", "static", prog), ("none", "dynamic", old), ("static", "none", was_static)):
        text = (f"trial 0: checkpoint {p['path']} was trained with --binarize {had}, "
                f"this run asks for --binarize {want}")
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            runner._check_resumed(p, spec, runner.RunOptions(binarize=want))
