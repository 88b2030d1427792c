"""The fused 28x28 launches take their tensors by slot name
(csrc/kernels/conv28_slots.h): the names, not a position in a list, decide
which kernel argument a tensor becomes, and a table that is wrong in any way
the host can see is a Python error before anything is launched.

B = 3, M = 2 (the smallest shape with a tail) on a trainer's own buffers.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, M = 3, 2
SENTINEL = 7.0
# the slots of every per-sample output of a training forward
OUTPUTS = ("xb", "a1", "a2", "mulv", "eps", "z16", "d0", "d1", "dlog", "bce_part", "kld_part", "db4_part")


@pytest.fixture(scope="module")
def tr(native_ext):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer

    t = ConvVaeTrainer(batch_size=B, image=28, device=torch.device("cuda"), backend="hip", seed=5, use_graphs=False)
    assert t.f28 and t.f28_merge and t.f28_pair
    g = torch.Generator().manual_seed(11)
    X = torch.rand(2 * B, 784, generator=g).cuda()
    idx = torch.randperm(2 * B, generator=g).to(torch.int32).cuda()
    t.bind_train_data(X, idx)
    t.set_cursor(0, 2)
    return t


def _fill_outputs(fwd, value):
    for k in OUTPUTS:
        fwd[k].fill_(value)


def _outputs(fwd):
    torch.cuda.synchronize()
    return {k: fwd[k].clone() for k in OUTPUTS}


def test_slot_names_are_the_builders_keys(tr):
    names = tr.C.f28_slot_names()
    assert set(names) == {"weights", "forward", "backward", "pair"}
    for k, v in names.items():
        assert len(set(v)) == len(v), k
    nw = len(names["weights"])
    assert nw == 12 and names["forward"][:nw] == names["weights"] and names["backward"][:nw] == names["weights"]
    p = tr._plan28(M)
    train, X, idx = p["fwd"], tr._data[0], tr._data[1]
    assert set(train) == set(names["forward"])
    assert train["xn"] is tr.f28_xn and train["xtag"] is tr.f28_xtag and train["state"] is tr.state.train_state
    ev = tr._eval_fwd28(X, idx, True)
    assert set(ev) <= set(names["forward"])
    assert ev.get("xn") is None and ev.get("xtag") is None and ev["state"] is tr.state.eval_state
    assert all(ev.get(k) is None for k in ("a1", "a2", "d0", "d1", "dlog", "stamps")) and ev["recon"] is tr.recon
    assert set(p["bwd"]) == set(names["backward"])
    assert set(tr._pair_table28()) == set(names["pair"])


def _bad_tables(tr, fwd):
    """(slot the error must name, forward table that is wrong in that slot)."""
    idx = fwd["idx"]
    return [("no_such_slot", dict(fwd, no_such_slot=tr.mulv)),                                    # an unknown key
            ("mulv", {k: v for k, v in fwd.items() if k != "mulv"}),                                # required, missing
            ("mulv", dict(fwd, mulv=None)),                                                         # required, None
            ("a1", dict(fwd, a1=torch.zeros(B * 6272, dtype=torch.float32, device="cuda"))),        # wrong dtype
            ("eps", dict(fwd, eps=tr.eps.view(-1)[:M * 32 - 1])),                                   # one element short
            ("idx", dict(fwd, idx=idx[:B + 1])),                                                    # no whole batches
            ("kld_part", dict(fwd, kld_part=torch.zeros(B)))]                                       # on the CPU


def test_a_wrong_table_is_an_error_that_names_the_slot_and_launches_nothing(tr):
    p = tr._plan28(M)
    fwd, C, stream = p["fwd"], tr.C, tr.rng_stream
    launches = {"f28_forward": lambda t: C.f28_forward(t, B, M, stream, True),
                "f28_step": lambda t: C.f28_step(t, p["bwd"], B, M, stream, pair=tr._pair_table28()),
                "f28_table": lambda t: C.f28_table("forward", t, B, M)}  # what the trainer's plan launches with
    _fill_outputs(fwd, SENTINEL)
    step = tr.read_state()["step"]
    for name, table in _bad_tables(tr, fwd):
        for what, launch in launches.items():
            with pytest.raises(RuntimeError, match=name):
                launch(table)
    # the backward and the pair table go through the same checks
    with pytest.raises(RuntimeError, match="gd1"):
        C.f28_backward({k: v for k, v in p["bwd"].items() if k != "gd1"}, M)
    with pytest.raises(RuntimeError, match="no_such_slot"):
        C.f28_step(fwd, p["bwd"], B, M, stream, pair=dict(tr._pair_table28(), no_such_slot=tr.f28_err))
    with pytest.raises(RuntimeError, match="pairw"):
        C.f28_step(fwd, p["bwd"], B, M, stream, pair=dict(tr._pair_table28(), pairw=None))
    # a table resolved for one launch shape is refused by another, and by a launch that wants another kind
    t = p["launch"]
    with pytest.raises(RuntimeError, match="forward table"):
        C.f28_forward(t["fwd"], B, M - 1, stream, True)
    with pytest.raises(RuntimeError, match="forward table"):
        C.f28_forward(t["fwd"], B, M, stream, False)
    with pytest.raises(RuntimeError, match="backward table"):
        C.f28_step(t["fwd"], t["fwd"], B, M, stream)
    for k, v in _outputs(fwd).items():
        assert bool((v == SENTINEL).all()), f"{k} was written by a call that raised"
    assert tr.read_state()["step"] == step and int(tr.f28_pairw.abs().sum()) == 0 and int(tr.f28_err.item()) == 0


def test_names_route_the_pointers_and_the_dict_form_is_the_trainers_step(tr):
    """a1 and d1 have one dtype and one size: no host check tells them apart.
    Exchanged by name, each lands in the other's buffer and nothing else moves.
    Then the correct table through ``f28_forward`` against ``train_steps``."""
    fwd, C, step = tr._plan28(M)["fwd"], tr.C, tr.read_state()["step"]
    assert fwd["a1"].dtype == fwd["d1"].dtype and fwd["a1"].numel() == fwd["d1"].numel()
    _fill_outputs(fwd, SENTINEL)
    C.f28_forward(fwd, B, M, tr.rng_stream, True)
    good = _outputs(fwd)
    assert not torch.equal(good["a1"], good["d1"])
    for k, v in good.items():
        rows = v.view(B, -1)
        assert bool((rows[M:] == SENTINEL).all()) and not bool((rows[:M] == SENTINEL).all()), k

    _fill_outputs(fwd, SENTINEL)
    C.f28_forward(dict(fwd, a1=fwd["d1"], d1=fwd["a1"]), B, M, tr.rng_stream, True)
    swapped = _outputs(fwd)
    assert torch.equal(swapped["a1"], good["d1"]) and torch.equal(swapped["d1"], good["a1"])
    for k in OUTPUTS:
        if k not in ("a1", "d1"):
            assert torch.equal(swapped[k], good[k]), k

    # neither launch advanced the step or the cursor: the trainer's own step runs on the same rows
    _fill_outputs(fwd, SENTINEL)
    tr.train_steps(1, M=M)
    own = _outputs(fwd)
    assert tr.read_state()["step"] == step + 1 and tr.health_error() is None
    for k in OUTPUTS:
        assert torch.equal(own[k], good[k]), k
