"""GPU: the two validators write their spectrogram pictures.

Inpainting: NPPCModelValidator.validate_batch(..., spectrograms=True) on the smallest ragged batch (B = 2: a 17-frame and an 18-frame gap), then
save_pc_spectrograms: the reference's file names, every file opens in Pillow at the size its item's context window gives,
output_spec.png holds the pixels of the alpha = 0 variation.

Speech enhancement: NPPCAudioValidator.visualize_pc_spectrograms on a 0.5 s clip writes the sheet and the reference's wav
names; and the sheet's `enhanced` panel, drawn from the spectrogram the committed fixture tests/golden/validator_f1.npz holds
(the reference's own enhanced STFT), lies within EPS levels of the fp64 restatement of that stored spectrogram (the dB
criterion of tests/test_spec_render_gpu.py).  Every test runs under a time limit of its own."""
import faulthandler
import os

import numpy as np
import pytest
import torch
from PIL import Image
from scipy.io import wavfile

import png_ref as R
from golden_util import GOLD, load
from oracle import weights as W

pytestmark = pytest.mark.gpu
LIMIT = 240
EPS = 2e-3


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- inpainting -------------------------------------------------------------------------------------------------------------------
NFFT, HOP, FQ, T64, KDIR = 63, 32, 32, 64, 3
GAPS = ((10, 17), (30, 18))                                        # (first frame, frames)
ALPHAS = (-1.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def inpainting_validator(tmp_path_factory):
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    tmp = tmp_path_factory.mktemp("val_png")
    wts = {k: torch.from_numpy(np.asarray(v)) for k, v in W.make_weights(W.inpainting_spec(KDIR), 41).items()}
    pre = "pretrained_restoration_model.net."
    ck = os.path.join(str(tmp), "restorer.pt")
    torch.save({"model_state_dict": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, ck)
    model_cfg = dict(
        pretrained_restoration_model_configuration=dict(in_channels=1, out_channels=1, dropout=0.2, precision="fp32"),
        pretrained_restoration_model_path=ck,
        audio_pc_wrapper_configuration=dict(n_dirs=KDIR, model_configuration=dict(in_channels=2, out_channels=KDIR, precision="fp32")),
        device="cuda")
    nppc = os.path.join(str(tmp), "nppc.pt")
    torch.save({"model_state_dict": wts}, nppc)
    val = V.NPPCModelValidator(V.NPPCModelValidatorConfig(checkpoint_path=nppc, save_dir=str(tmp / "val"),
                                                          model_configuration=model_cfg))
    g = torch.Generator().manual_seed(11)
    clean = torch.randn(2, 2, FQ, T64, generator=g)
    mask = torch.ones(2, T64)
    for b, (s, n) in enumerate(GAPS):
        mask[b, s:s + n] = 0
    return V, val, (clean * mask[:, None, None, :], mask, clean), tmp


def test_inpainting_validator_writes_the_reference_file_names(inpainting_validator):
    V, val, batch, tmp = inpainting_validator
    with pytest.raises(ValueError, match="same number of masked"):
        val.validate_batch(*batch, n_mc_samples=4, n_components=KDIR)
    plain = val.validate_batch(*batch, n_mc_samples=4, n_components=KDIR, ragged_gaps=True)
    assert "masked_spec_mag_norm" not in plain                     # the default returns the keys it always returned
    with pytest.raises(ValueError, match="spectrograms=True"):
        V.save_pc_spectrograms(plain, tmp / "none", ALPHAS)
    out = val.validate_batch(*batch, n_mc_samples=4, n_components=KDIR, ragged_gaps=True, spectrograms=True)
    assert set(out) - set(plain) == {"masked_spec_mag_norm"}
    assert out["masked_spec_mag_norm"].shape == out["clean_spec_mag_norm"].shape == (2, 1, FQ, T64)
    sx, sy, gut = 2, 3, 4
    paths = V.save_pc_spectrograms(out, tmp / "spec", ALPHAS, first_index=5, sx=sx, sy=sy, gutter=gut)
    names = ["clean_spec.png", "masked_spec.png", "output_spec.png", "error_spec.png"]
    for k in range(1, KDIR + 1):
        names += [f"pc_direction_{k}.png"] + [f"pc{k}_alpha_{a:.1f}.png" for a in ALPHAS]
    names.append("sheet.png")
    want = [tmp / "spec" / f"sample_{5 + b}" / "spectrograms" / n for b in range(2) for n in names]
    assert [str(p) for p in paths] == [str(p) for p in want]
    assert sorted(str(p) for p in (tmp / "spec").rglob("*") if p.is_file()) == sorted(str(p) for p in want)
    assert (tmp / "spec" / "sample_6" / "spectrograms" / "pc3_alpha_-1.0.png").exists()
    widths = [R.window(batch[1][b].numpy()) for b in range(2)]
    assert [w[1] - w[0] for w in widths] == [44, 52]               # 17 + 17 + 10 frames (clamped at 0), 18 + 18 + 16 (at T)
    for b in range(2):
        t0, t1, m0, m1 = widths[b]
        d = tmp / "spec" / f"sample_{5 + b}" / "spectrograms"
        w = (t1 - t0) * sx
        panels = {}
        for n in names[:-1]:
            im = Image.open(d / n)
            assert im.mode == "P" and im.size == (w, FQ * sy), n
            panels[n] = np.asarray(im)
        sheet = Image.open(d / "sheet.png")
        assert sheet.size == (6 * w + 5 * gut, (1 + KDIR) * FQ * sy + KDIR * gut)
        assert np.array_equal(panels["output_spec.png"], panels["pc1_alpha_0.0.png"])
        assert np.array_equal(panels["output_spec.png"], panels["pc3_alpha_0.0.png"])
        assert not np.array_equal(panels["output_spec.png"], panels["pc1_alpha_1.0.png"])
        # the panels against the restatement of the validator's own tensors: exact
        from nppc_audio.spectrogram_png import Cell, Sheet
        x = torch.cat([out["clean_spec_mag_norm"], out["masked_spec_mag_norm"], out["pred_spec_mag_norm"], out["pc_directions"]],
                      dim=1).float().cpu().numpy()
        for n, cell in (("clean_spec.png", Cell(p=0, vmin=-3.0, vmax=3.0, markers=True)),
                        ("error_spec.png", Cell(p=0, q=2, alpha=-1.0, g="abs", vmin=0.0, vmax=3.0, markers=True)),
                        ("pc2_alpha_-1.0.png", Cell(p=2, q=4, alpha=-1.0, vmin=-3.0, vmax=3.0, markers=True))):
            assert np.array_equal(panels[n], R.render(x, Sheet(b, [[cell]], sx=sx, sy=sy), widths[b])), (b, n)
        # the sheet: its cell (0, 2) is the output panel without markers, its cell (1, 2) the alpha = 0 variation with them
        s = np.asarray(sheet)
        plain = R.render(x, Sheet(b, [[Cell(p=2, vmin=-3.0, vmax=3.0)]], sx=sx, sy=sy), widths[b])
        assert np.array_equal(s[:FQ * sy, 2 * (w + gut):2 * (w + gut) + w], plain)
        y0 = FQ * sy + gut
        assert np.array_equal(s[y0:y0 + FQ * sy, 2 * (w + gut):2 * (w + gut) + w], panels["output_spec.png"])
        assert (s[:, w:w + gut] == 255).all() and (s[FQ * sy:y0] == 255).all()
        assert (panels["clean_spec.png"][:4, (m0 - t0) * sx] == 254).all()
    # without the individual panels, fewer directions, the gray palette
    only = V.save_pc_spectrograms(out, tmp / "sheets", ALPHAS, individual=False, max_dirs=2, sx=1, sy=1, palette="gray")
    assert [p.name for p in only] == ["sheet.png"] * 2
    assert Image.open(only[0]).size == (6 * 44 + 5 * 4, 3 * FQ + 2 * 4)


def test_validate_dataloader_can_write_the_spectrograms(inpainting_validator):
    V, val, batch, tmp = inpainting_validator
    res = val.validate_dataloader([batch], n_mc_samples=4, n_components=KDIR, save=True, ragged_gaps=True, spectrogram_alphas=ALPHAS)
    assert res["n_items"] == 2
    for i in range(2):
        d = tmp / "val" / f"sample_{i}" / "spectrograms"
        assert (d / "sheet.png").exists() and (d / "pc_direction_3.png").exists()
        assert (tmp / "val" / "validation_metrics" / f"sample_{i}.json").exists()


# ---- speech enhancement -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def audio_validator(tmp_path_factory):
    from nppc_audio.validator import NPPCAudioValidator, NPPCAudioValidatorConfig
    tmp = tmp_path_factory.mktemp("se_val_png")
    _, meta = load("g1_c1")
    c = meta["config"]
    spec = W.nppc_spec(c["K"], num_freqs=c["F"], sb_neighbors=c["sbn"], sb_hidden=c["sbh"])
    wts = {k: torch.from_numpy(v) for k, v in W.make_weights(spec, c["seed"]).items()}
    pre = "pretrained_restoration_model."
    ck = os.path.join(str(tmp), "restorer.tar")
    torch.save({"model": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, ck)
    common = dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"], precision="fp32")
    model_cfg = dict(
        pretrained_restoration_model_configuration=dict(common, num_groups_in_drop_band=c["G_rest"]),
        pretrained_restoration_model_path=ck,
        audio_pc_wrapper_configuration=dict(multi_direction_configuration=dict(common, num_groups_in_drop_band=c["G_pc"],
                                                                               n_directions=c["K"])),
        stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"]), device="cuda")
    nppc = os.path.join(str(tmp), "nppc.pt")
    torch.save({"model_state_dict": wts, "step": 0}, nppc)
    return NPPCAudioValidator(NPPCAudioValidatorConfig(nppc_audio_model_configuration=model_cfg, checkpoint_path=nppc)), c, tmp


def test_audio_validator_writes_the_sheet_and_the_reference_wav_names(audio_validator):
    from nppc_audio import validator as AV
    val, c, tmp = audio_validator
    noisy, clean = W.synth_batch(1, 8000)                          # 0.5 s
    F, T = c["F"], 1 + 8000 // c["hop"]
    specs, enh_db = val.visualize_pc_spectrograms(torch.from_numpy(noisy), torch.from_numpy(clean), tmp / "one")
    assert len(specs) == c["K"] and all(s.shape == (1, F, T) and s.is_complex() for s in specs) and enh_db.shape == (1, F, T)
    wavs = ["noisy.wav", "clean.wav", "enhanced.wav"] + [f"pc{k}_alpha{a:.1f}.wav" for k in range(c["K"]) for a in AV.ALPHAS]
    assert f"pc1_alpha-1.8.wav" in wavs and len(wavs) == 3 + 6 * c["K"]
    files = sorted(str(p.relative_to(tmp / "one")) for p in (tmp / "one").rglob("*") if p.is_file())
    assert files == sorted([os.path.join("audio", w) for w in wavs] + [os.path.join("spectrograms", "pc_spectrograms_variations.png")])
    for w in wavs:
        sr, x = wavfile.read(str(tmp / "one" / "audio" / w))
        assert sr == 16000 and x.dtype == np.int16 and x.shape == (8000,) and np.abs(x.astype(np.int32)).max() >= 32766, w
    sheet = Image.open(tmp / "one" / "spectrograms" / "pc_spectrograms_variations.png")
    gut = 4
    assert sheet.mode == "P" and sheet.size == (9 * T + 8 * gut, (1 + c["K"]) * F + c["K"] * gut)
    s = np.asarray(sheet)
    assert (s[:F, 4 * (T + gut):] == 255).all() and (s[F + gut:2 * F + gut, 7 * (T + gut):] == 255).all()     # blank cells
    assert s[:F, :T].max() == 253 and s[:F, :T].min() == 0                                                       # autoscaled
    e = s[:F, 2 * (T + gut):2 * (T + gut) + T]
    assert e.max() == 253 and e.min() == 0 and np.isfinite(enh_db.cpu().numpy()).all()
    # without clean audio: no clean.wav, the clean and error cells are blank; a batch of two: one folder per item
    val.visualize_pc_spectrograms(torch.from_numpy(np.concatenate([noisy, noisy[:, ::-1].copy()])), None, tmp / "two")
    assert not (tmp / "two" / "item_0" / "audio" / "clean.wav").exists() and (tmp / "two" / "item_1" / "audio" / "pc0_alpha3.0.wav").exists()
    s2 = np.asarray(Image.open(tmp / "two" / "item_0" / "spectrograms" / "pc_spectrograms_variations.png"))
    assert (s2[:F, T + gut:2 * T + gut] == 255).all() and (s2[:F, 3 * (T + gut):] == 255).all()
    assert np.array_equal(s2[:F, :T], s[:F, :T])                                                                # the same noisy panel


def test_enhanced_panel_matches_the_restatement_of_the_stored_reference_spectrogram(audio_validator):
    from nppc_audio import ops
    from nppc_audio import validator as AV
    val, c, _ = audio_validator
    z, _ = load("g1_c1")
    v = np.load(os.path.join(GOLD, "validator_f1.npz"))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _, c_re, c_im = ops.stft(dev(z["clean"]), c["nfft"], c["hop"], want_mag=False)
    planes = AV.stack_planes((dev(z["noisy_real"][:, 0]), dev(z["noisy_imag"][:, 0])), (c_re, c_im),
                             (dev(v["enhanced_re"]), dev(v["enhanced_im"])), (dev(v["w_spec_re"]), dev(v["w_spec_im"])))
    B, F, T = v["enhanced_re"].shape
    sheets = val.pc_spectrogram_indices(planes)
    host = planes.cpu().numpy()
    from nppc_audio.spectrogram_png import Cell
    worst = 0.0
    for b in range(B):
        s = sheets[b].cpu().numpy().astype(np.float64)
        assert s.shape == ((1 + c["K"]) * F + c["K"] * 4, 9 * T + 8 * 4)
        for (r, col), cell in {(0, 2): Cell(p=AV.ENHANCED, g="db"),
                               (0, 3): Cell(p=AV.ENHANCED, q=AV.CLEAN, alpha=-1.0, g="db", vmin=-60.0, vmax=0.0),
                               (1, 0): Cell(q=AV.PC, g="db", vmin=-60.0, vmax=0.0),
                               (2, 4): Cell(p=AV.ENHANCED, q=AV.PC + 1, alpha=AV.ALPHAS[3], g="db")}.items():
            pos, _, _ = R.positions(host, b, cell, 0, T)
            pos = np.clip(pos[::-1], 0.0, 254.0)
            idx = s[r * (F + 4):r * (F + 4) + F, col * (T + 4):col * (T + 4) + T]
            worst = max(worst, float(np.maximum(idx - pos, pos - (idx + 1)).max()))
    print(f"enhanced / error / PC / variation panels of the stored spectrograms: largest excess {worst:.3e} levels")
    assert worst <= EPS, worst
