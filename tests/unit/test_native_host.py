"""Host-side native runtime on CPU: the conv planners of csrc/runtime/conv_ops.cpp
(tile / split-K / wgrad grid choices) for every layer of both conv-VAEs at
awkward batch sizes. Runs in the normal CPU suite and under the ASan/UBSan
build (scripts/sanitize_host.sh, MDT_NATIVE_SO=build/san/_C.so), where an
out-of-bounds table access or signed overflow in a planner aborts the test."""
import pytest

from multidisttorch_amd.ops import conv_plans as plans
from multidisttorch_amd.ops import native

pytestmark = pytest.mark.skipif(not native.available(), reason="native extension not built")


def _descs(image, M):
    from multidisttorch_amd.models.conv_vae import ConvVaeTrainer, conv_vae_spec

    spec = conv_vae_spec(image, 1, 32 if image == 28 else 64)
    return [(l, ConvVaeTrainer._desc(l, M)) for l in spec]


@pytest.mark.parametrize("image", [28, 128])
@pytest.mark.parametrize("M", [1, 7, 64, 128, 129, 1000])
def test_conv_planners_consistent(image, M):
    C = native.require()
    for l, d in _descs(image, M):
        if l.cin == 1 or l.cout == 1:
            nb = C.thin_blocks(l.kind == "convT", d)
            assert nb > 0
            if l.kind != "convT":
                continue
        modes = [0, 1]
        for mode in modes:
            for split in (False, True):
                try:
                    q = plans.igemm_plan(mode, d, split)
                except RuntimeError as e:
                    assert "unsupported geometry" in str(e)
                    continue
                classes, rows, ncols, K, ks, csrows = q.classes, q.m, q.ncols, q.k, q.ksplit, q.colsum_rows
                assert classes >= 1 and rows >= 1 and ncols >= 1 and K >= 1
                assert ks >= 1 and (split or ks == 1)
                assert csrows >= 1
        w = plans.wgrad_plan(d)
        assert w.nsplit >= 1  # m-splits (partial slabs)
        assert all(v >= 0 for v in w)
    for ks in (1, 2, 8):
        assert C.combine_reparam_blocks(ks, M, 32) >= 1


@pytest.mark.parametrize("M", [1, 7, 64, 128])
def test_thin_mfma_wgrad_plan(M):
    """The single-channel 128x128 layers (enc1, and the last layer in its conv
    view) plan the MFMA weight gradient (conv_thin_wg.h, cfg 110): one partial
    row per 4 output rows, i.e. M * 64 / 4 slabs of [32][16]; the 28x28 edge
    layers keep the generic thin weight gradient."""
    import os

    C = native.require()
    if os.environ.get("MDT_THIN_MFMA", "15") not in ("14", "15"):
        pytest.skip("non-default MDT_THIN_MFMA mask")
    for image in (28, 128):
        for l, d in _descs(image, M):
            if not (l.cin == 1 or l.cout == 1):
                continue
            info = plans.wgrad_plan(d)
            if image == 128:
                assert (info.cfg == plans.WG_THIN_MFMA and info.nsplit == M * 64 // 4 and info.bm == 32
                        and info.bn == 16), info
            else:
                assert info.cfg != plans.WG_THIN_MFMA, info


@pytest.mark.parametrize("args,msg", [
    ((32, 64, 64, 10), r"latent size Z = 10 must be a multiple of 4 in \[4, 32\]"),
    ((32, 64, 64, 36), r"latent size Z = 36"),
    ((32, 64, 402, 8), r"hidden size H = 402 must be a positive multiple of 4"),
    ((32, 64, 516, 8), r"hidden size H = 516 exceeds the limit of 512"),
    ((32, 30, 64, 8), r"input size D = 30 must be a positive multiple of 4"),
    ((4097, 64, 64, 8), r"batch size 4097 must be in \[1, 4096\]"),
    ((512, 16384, 64, 8), r"needs 131072 BCE partial slots .* limit 65536"),
])
def test_mlp_engine_refuses_unsupported_shapes_by_name(args, msg):
    """MlpVaeEngine's shape checks (docs/KERNELS.md, "MLP-VAE shape domain") come
    before any allocation, so they hold on a host without a GPU too."""
    with pytest.raises(RuntimeError, match=msg):
        native.require().MlpVaeEngine(*args, 0)
