"""Host side of the VAE threshold tests: the tables of tests/_vae_cases.py are the batch sizes the committed scans list
(profiles/plan_thresholds_vae_<tag>.txt, written by tools/plan_thresholds.py), every one of them is run on both sides, no case is
marked away, and the float64 references treat every sample on its own, so that a per-sample comparison against them means what it
says."""
import os

import pytest
import torch

from tests import _vae_cases as V
from tests import test_gpu_vae_thresholds as G
from tests._plan_sig import read_scan


def test_the_tags_cover_both_directions_of_every_shape():
    assert set(V.TAGS) == set(V.THRESHOLDS) == {f"{d}_{s}" for d in ("dec", "enc") for s in V.SHAPES}
    assert V.SHAPES["batch"][0] == dict(block_out_channels=(128, 256), layers_per_block=1) and V.SHAPES["batch"][1] == (8, 32)
    assert V.scanned_to("dec_batch") == 130 and V.image_hw("enc_batch") == (16, 64)
    assert set(V.SHAPE_SWEEP) == {"8x64", "16x32", "8x16", "6x26"}
    for s in V.SHAPE_SWEEP:
        cfg, (h, w), top_dec, top_enc = V.SHAPES[s]
        assert cfg == dict(block_out_channels=(64, 64, 128, 128), layers_per_block=1) and f"{h}x{w}" == s and top_dec == top_enc == 16
        assert V.image_hw("enc_" + s) == (8 * h, 8 * w)
    from worddiffusion_amd.vae import AutoencoderKL
    assert V.ENCODE_CHUNK == AutoencoderKL.ENCODE_CHUNK
    assert all(V.scanned_to(t) <= V.ENCODE_CHUNK for t in V.TAGS if t.startswith("enc_"))  # (the encoder plans nothing larger)


@pytest.mark.parametrize("tag", V.TAGS)
def test_the_tables_are_the_committed_scans(tag):
    path = V.scan_file(tag)
    assert os.path.basename(path) == f"plan_thresholds_vae_{tag}.txt"
    with open(path) as f:
        head = f.readline()
    assert head.startswith("# plan thresholds: ") and V.scan_header(tag) in head and "(tools/plan_thresholds.py)" in head, head
    scan = read_scan(path)
    assert list(scan) == sorted(scan) and min(scan) >= 2 and max(scan) <= V.scanned_to(tag)
    assert V.THRESHOLDS[tag] == tuple(scan), f"re-run `{V.scan_command(tag)}` and copy its B column into THRESHOLDS"
    assert max(scan) <= V.pool_size(tag)


@pytest.mark.parametrize("tag", V.TAGS)
def test_no_threshold_is_dropped_from_the_cases(tag):
    """Every listed b is a case of the cross-threshold test, b - 1 and b are both cases of the oracle test, each once; every shape tag
    also runs B = 1, 2, 3 and every encoder tag the full chunk."""
    scan = read_scan(V.scan_file(tag))
    assert [b for t, b in V.THRESHOLD_CASES if t == tag] == list(scan)
    ran = [B for t, B in V.ORACLE_CASES if t == tag]
    want = {B for b in scan for B in (b - 1, b)}
    if V.split(tag)[1] in V.SHAPE_SWEEP:
        want |= {1, 2, 3}
    if tag.startswith("enc_"):
        want.add(16)
    assert len(ran) == len(set(ran)) and set(ran) == want and tuple(ran) == V.batch_sizes(tag)
    assert min(ran) >= 1 and V.pool_size(tag) == max(ran)


def test_no_case_is_marked_away():
    fns = {G.test_matches_the_reference_on_both_sides_of_a_threshold: V.ORACLE_CASES,
           G.test_a_sample_keeps_its_value_across_a_threshold: V.THRESHOLD_CASES,
           G.test_every_listed_threshold_changes_the_plan: V.TAGS}
    for fn, cases in fns.items():
        marks = [mk for mk in fn.pytestmark if mk.name == "parametrize"]
        assert len(marks) == 1 and list(marks[0].args[1]) == list(cases), fn.__name__
        assert all(not hasattr(c, "marks") for c in marks[0].args[1]), fn.__name__   # (no pytest.param(..., marks=...))
    every = list(fns) + [G.test_encode_chunking_at_the_real_chunk_size]
    assert all(mk.name in ("parametrize", "gpu") for fn in every for mk in getattr(fn, "pytestmark", []))
    assert G.pytestmark.name == "gpu"
    assert {t for t, _ in V.ORACLE_CASES} == {t for t, _ in V.THRESHOLD_CASES} == set(V.TAGS)
    assert G.ORACLE_BAR == 1e-4 and G.CROSS_BAR == 5e-5


def test_the_expected_thresholds_are_in_the_batch_scans():
    """What reading ``wd_auto_tile`` / ``wd_auto_ksplit`` suggests for the (128, 256) decoder at 8 x 32 is among what the scan found:
    post_quant_conv (n = 4, one K stage, no cut) leaves the 64 x 64 tile when ceil(256 B / 128) reaches 128; the 256-channel 3x3
    layers (36 K stages, cap 8, 4 B tiles) step 8 -> 7 -> 6 -> 5 -> 4 -> 3 -> 2 and drop the cut at 33 (32 is exactly 128 tiles with
    >= 32 stages: still cut); the 128-channel layers at 1024 positions (8 B tiles) step at 9 and 11 and drop the cut at 16."""
    scan = read_scan(V.scan_file("dec_batch"))
    assert {9, 10, 11, 13, 16, 17, 22, 33, 64} <= set(scan) and 32 not in scan
    assert scan[64] == ("post_quant_conv: wd_gemm K_V2 w_layout=0 tile=64064 ksplit=1 nsrc=1 [f32] -> "
                        "wd_gemm K_V2 w_layout=0 tile=128064 ksplit=1 nsrc=1 [f32]")
    for b, (k0, k1) in {9: (8, 7), 10: (7, 6), 11: (6, 5), 13: (5, 4), 17: (4, 3), 22: (3, 2), 33: (2, 1)}.items():
        assert f"mid.r0.conv1, mid.r0.conv2, mid.r1.conv1 (+5 more): wd_gemm K_V2 w_layout=0 tile=128128 ksplit={k0} nsrc=1 [stat f32] -> " \
               f"wd_gemm K_V2 w_layout=0 tile=128128 ksplit={k1} nsrc=1 [stat f32]" in scan[b], b
    for b, (k0, k1) in {9: (4, 3), 11: (3, 2), 16: (2, 1)}.items():
        assert f"up1.r1.conv1, up1.r1.conv2: wd_gemm K_V2 w_layout=0 tile=128128 ksplit={k0} nsrc=1 [stat f32] -> " \
               f"wd_gemm K_V2 w_layout=0 tile=128128 ksplit={k1} nsrc=1 [stat f32]" in scan[b], b
    # every VAE GEMM of every scan is on the forced 128 x 128 tile, except the two im2col-fed and the output convolutions
    for tag in V.TAGS:
        for b, text in read_scan(V.scan_file(tag)).items():
            for part in text.split("; "):
                if not part.startswith(("post_quant_conv", "decoder.conv_out", "encoder.conv_out")):
                    assert part.count("tile=128128") == 2, (tag, b, part)


def test_pool_samples_are_distinct_scaled_and_stable():
    for tag in ("dec_8x16", "enc_6x26"):
        x = V.pool_inputs(tag)
        assert x.shape == ((V.pool_size(tag), 4, *V.latent_hw(tag)) if tag.startswith("dec") else (V.pool_size(tag), 3, *V.image_hw(tag)))
        assert x.dtype == torch.float32 and torch.equal(V.pool_inputs(tag, 3), x[:3])
        amax = [float(x[b].abs().max()) for b in range(6)]
        if tag.startswith("enc"):  # images in [-1, 1], then the per-sample scale
            assert all(a <= V.SAMPLE_SCALE[b % 3] for b, a in enumerate(amax)) and amax[1] <= 0.5 < amax[0] <= 1.0 < amax[2]
        else:
            std = [float(x[b].std()) for b in range(6)]
            assert all(abs(s / (3.0 * V.SAMPLE_SCALE[b % 3]) - 1) < 0.2 for b, s in enumerate(std)), std
    assert not torch.equal(V.pool_inputs("dec_8x16", 1), V.pool_inputs("dec_batch", 1)[:, :, :, :16])


@pytest.mark.parametrize("tag", ["dec_8x16", "enc_8x16", "dec_batch", "enc_batch"])
def test_the_references_treat_every_sample_on_its_own(tag):
    """The pool's first 3 samples run together equal the same samples run one by one to <= 1e-12 relative (float64)."""
    _, sd = V.build_model(tag)
    x = V.pool_inputs(tag, 3)
    together = V.reference(tag, sd, x)
    single = V.reference(tag, sd, x, chunk=1)
    if tag.startswith("dec"):
        together, single = (together,), (single,)
    for t, s in zip(together, single):
        assert t.dtype == torch.float64 and t.shape[0] == 3
        for b in range(3):
            assert float((t[b] - s[b]).abs().max() / s[b].abs().max()) <= 1e-12, (tag, b)
        assert float((t[0] - t[1]).abs().max()) > 1e-3   # (and the samples do differ)
