"""CPU: the inpainting validator's oracle against torch.istft, the host half of compute_metrics_batch against the
reference's compute_metrics fixture, and the argument checks of the new C entry points (no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import inpaint_validator_ref as VR
from oracle import inpaint_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = [(255, 128), (254, 127), (100, 25), (512, 256)]


def planes(B, n_fft, T, seed):
    g = torch.Generator().manual_seed(seed)
    F = n_fft // 2 + 1
    return torch.randn(B, F, T, generator=g), torch.randn(B, F, T, generator=g)


@pytest.mark.parametrize("n_fft,hop", CONFIGS)
def test_oracle_istft_equals_torch_istft_in_fp64(n_fft, hop):
    for T in (2, 9, 37):
        re, im = planes(2, n_fft, T, n_fft + T)
        nat = VR.natural_length(n_fft, hop, T)
        assert nat == hop * (T - 1) + (n_fft % 2)
        for length in (None, nat - 3, max(1, nat - n_fft - 5), nat + 7):
            want = VR.torch_istft(re, im, n_fft, hop, length).numpy()
            got = VR.istft(re, im, n_fft, hop, length)
            assert got.shape == want.shape == (2, nat if length is None else length)
            assert np.abs(got - want).max() < 1e-12 * np.abs(want).max(), (n_fft, hop, T, length)


def test_natural_lengths_of_the_inpainting_configuration():
    for T, L in ((9, 1025), (37, 4609), (500, 63873)):
        re, im = planes(1, 255, T, T)
        assert VR.torch_istft(re, im, 255, 128).shape[-1] == L == VR.natural_length(255, 128, T)
    from nppc_audio import ops
    assert ops.istft_natural_length(255, 128, 500) == 63873 and ops.istft_natural_length(254, 127, 9) == 127 * 8


@pytest.mark.parametrize("n_fft,hop", CONFIGS)
def test_imaginary_dc_and_nyquist_are_ignored(n_fft, hop):
    re, im = planes(1, n_fft, 9, 5)
    im2 = im.clone()
    im2[:, 0] = 7.0
    if n_fft % 2 == 0:
        im2[:, -1] = -3.0
    assert np.array_equal(VR.istft(re, im, n_fft, hop), VR.istft(re, im2, n_fft, hop))
    assert torch.equal(VR.torch_istft(re, im, n_fft, hop), VR.torch_istft(re, im2, n_fft, hop))


def test_envelope_helper_matches_torch_refusal():
    from nppc_audio import ops
    assert ops.istft_envelope_min(255, 128, 9, 1025) > 1e-11
    assert ops.istft_envelope_min(64, 64, 4, 192) < 1e-11            # hop = n_fft: the hann window's zero is never covered
    re, im = planes(1, 64, 4, 1)
    with pytest.raises(RuntimeError, match="window overlap add min"):
        VR.torch_istft(re, im, 64, 64)


def stacked_fixture():
    """both cases of tests/golden/metrics.npz as ONE batch of two.  Case a is n = 5 on 16 x 25, case b n = 3 on 32 x 40;
    b gets two all-zero directions per set and a gets zero elements (mask 1, pred = mean = clean = 0) up to 1280: a zero
    element adds nothing to any inner product, and a zero direction has no component in the error and no eigenvalue above
    the whitening threshold, so every metric of either item is what it is alone."""
    z = np.load(os.path.join(GOLD, "metrics.npz"))
    n, N = 5, 32 * 40
    out = {k: [] for k in ("nppc", "mc", "pred", "mean", "clean", "mask")}
    for case in ("a", "b"):
        for k in out:
            x = z[f"{case}_{k}"].astype(np.float32)
            x = x.reshape(x.shape[1], -1)
            rows = n if k in ("nppc", "mc") else 1
            full = np.ones((rows, N), np.float32) if k == "mask" else np.zeros((rows, N), np.float32)
            if k == "mask":
                full[:, :x.shape[1]] = x
            else:
                full[:x.shape[0], :x.shape[1]] = x
            out[k].append(full)
    return z, {k: np.stack(v) for k, v in out.items()}, n


def check_against_fixture(z, case, m):
    got = np.array([m["nppc"]["rmse"], m["nppc"]["residual_error"], m["mc_dropout"]["rmse"], m["mc_dropout"]["residual_error"]])
    assert np.abs(got - z[f"{case}_scalars"]).max() < 2e-6 * z[f"{case}_scalars"].max()
    ang = np.array(m["principal_angles"])
    assert ang.shape == z[f"{case}_angles"].shape
    assert np.abs(ang - z[f"{case}_angles"]).max() < 1e-3


def test_host_half_of_compute_metrics_batch_on_the_stacked_fixture():
    from nppc_audio.inpainting.mc_baseline import metrics_from_gram
    z, t, n = stacked_fixture()
    G = np.stack([VR.gram(VR.metric_rows(*(t[k][b][None] for k in ("nppc", "mc", "pred", "mean", "clean", "mask"))))
                  for b in range(2)])
    assert G.shape == (2, 13, 13)
    ms = metrics_from_gram(G, n)
    assert len(ms) == 2
    for case, m in zip("ab", ms):
        check_against_fixture(z, case, m)
        o = R.compute_metrics(*(torch.from_numpy(z[f"{case}_{k}"]).double() for k in ("nppc", "mc", "pred", "mean", "clean", "mask")))
        got = np.array([m["nppc"]["rmse"], m["nppc"]["residual_error"], m["mc_dropout"]["rmse"], m["mc_dropout"]["residual_error"]])
        want = np.array([o["nppc"]["rmse"], o["nppc"]["residual_error"], o["mc_dropout"]["rmse"], o["mc_dropout"]["residual_error"]])
        assert np.abs(got - want).max() < 2e-6 * want.max()
        assert np.abs(np.array(m["principal_angles"]) - np.array(o["principal_angles"])).max() < 1e-3
    one = metrics_from_gram(G[1], n)                                 # a single matrix is a batch of one
    assert one[0] == ms[1]
    with pytest.raises(ValueError, match="Gram"):
        metrics_from_gram(G, 3)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from nppc_audio import _hip
    fake = ctypes.c_void_p(4096)                                     # never dereferenced: the checks come before any launch
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_istft_any", None, None, 128 * 9, None, 1025, 1, 9, 255, 128, 1025, None)
    with pytest.raises(RuntimeError, match="bad argument"):          # hop = n_fft: envelope below 1e-11 inside the kept range
        _hip.call("nppc_istft_any", fake, fake, 33 * 4, fake, 192, 1, 4, 64, 64, 192, None)
    with pytest.raises(RuntimeError, match="unsupported"):
        _hip.call("nppc_istft_any", fake, fake, 513 * 4, fake, 1024, 1, 4, 1024, 256, 768, None)
    with pytest.raises(RuntimeError, match="unsupported"):           # ceil(n_fft / hop) = 9 frames over one sample
        _hip.call("nppc_istft_any", fake, fake, 51 * 40, fake, 400, 1, 40, 100, 12, 400, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_pc_variation_waves", None, None, None, None, None, None, None, None, None, 1, 5, 13, 9, 255, 128, 1025, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_pc_variation_waves", fake, fake, fake, fake, fake, fake, fake, fake, fake, 1, 5, 13, 4, 64, 64, 192, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        _hip.call("nppc_metrics_batch", None, None, None, None, None, None, None, 2, 5, 1280, None)
    with pytest.raises(RuntimeError, match="unsupported"):
        _hip.call("nppc_metrics_batch", fake, fake, fake, fake, fake, fake, fake, 2, 9, 1280, None)


def test_validator_surface_imports_and_fails_loudly_without_a_gpu(tmp_path):
    from nppc_audio.inpainting.trainer.nppc_trainer import NPPCAudioInpaintingTrainer
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    assert callable(NPPCAudioInpaintingTrainer.validate)
    assert set(V.NPPCModelValidatorConfig.model_fields) == {"checkpoint_path", "device", "save_dir", "model_configuration",
                                                            "max_dirs_to_plot"}
    assert torch.equal(V.default_alphas(), torch.arange(-3, 3.5, 0.5)) and V.default_alphas().numel() == 13
    m = {"nppc": {"rmse": 1.0, "residual_error": np.float64(0.5)}, "mc_dropout": {"rmse": 2.0, "residual_error": 0.25},
         "principal_angles": [10.0, 20.0]}
    V.save_metrics_to_json(m, tmp_path, 3)
    import json
    got = json.load(open(tmp_path / "validation_metrics" / "sample_3.json"))
    assert got == {"nppc": {"rmse": 1.0, "residual_error": 0.5}, "mc_dropout": {"rmse": 2.0, "residual_error": 0.25},
                   "principal_angles": [10.0, 20.0]}
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP"):
            V.pc_audio_variations(torch.zeros(1, 1, 128, 9), torch.zeros(1, 1, 128, 9), torch.zeros(1, 5, 128, 9),
                                  torch.zeros(1, 2, 128, 9), V.default_alphas(), 0.0, 1.0)
