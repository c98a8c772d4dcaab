"""GPU: the two validators write their pitch figures.

Inpainting: NPPCModelValidator.validate_batch(..., pitch=True) on the tiny fixture, then save_pc_pitch_plots: the reference's
tree of file names, every file opens in Pillow, and the index image of a direction's figure and of the stacked figure equal
the restatement tests/curve_ref.py fed with the dict's own contours and the gap markers worked out here from the mask.
Speech enhancement: NPPCAudioValidator.visualize_pc_pitch writes pitch/pc_<k>_pitch.png and pitch/pitch_comparison.png, equal
to the restatement of the contours it returns.  Every test runs under a time limit of its own."""
import faulthandler
import os

import numpy as np
import pytest
import torch
from PIL import Image

import curve_ref as R
from oracle import weights as W

pytestmark = pytest.mark.gpu
LIMIT = 240


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def test_inpainting_validator_writes_the_pitch_figures(tmp_path):
    from nppc_audio import curve_png as CP
    from nppc_audio.inpainting.validator import validator_nppc_model as V
    from test_inpaint_gpu import build_trainer, load
    from test_inpaint_validator_gpu import held_out
    z, meta = load("inp_tiny")
    c = meta["config"]
    tr, _, _ = build_trainer(meta, "fp32", tmp_path, z)
    ck = str(tmp_path / "out" / "nppc.pt")
    tr.save_checkpoint(ck)
    val = V.NPPCModelValidator(V.NPPCModelValidatorConfig(checkpoint_path=ck, save_dir=str(tmp_path / "val"),
                                                          model_configuration=tr.config.nppc_model_configuration.model_dump()))
    b = held_out(z, 3)
    alphas = V.default_alphas()
    kw = dict(n_mc_samples=8, n_components=c["K"], alphas=alphas, n_fft=c["nfft"], hop_length=c["hop"])
    with pytest.raises(ValueError, match="pitch=True"):
        V.save_pc_pitch_plots(val.validate_batch(*b, **kw), tmp_path / "none", alphas)
    out = val.validate_batch(*b, pitch=True, **kw)
    f0 = out["pitch"]["f0"]
    B, K, A, T = f0.shape
    sx, PH = 3, 50
    paths = V.save_pc_pitch_plots(out, tmp_path / "pitch", alphas, first_index=4, sx=sx, plot_height=PH, hop_length=c["hop"])
    want = []
    for i in range(B):
        want += [tmp_path / "pitch" / f"sample_{4 + i}" / "pitch_contours" / f"pc_{k}_pitch.png" for k in range(1, K + 1)]
        want.append(tmp_path / "pitch" / f"sample_{4 + i}" / "pitch_comparison.png")
    assert [str(p) for p in paths] == [str(p) for p in want]
    assert sorted(str(p) for p in (tmp_path / "pitch").rglob("*") if p.is_file()) == sorted(str(p) for p in want)
    # the restatement of the dict's own contours; the markers by hand: STFT frame f -> (f hop + 256) // 512
    values = CP.stack_contours(out["pitch"]).cpu().numpy()
    mask = out["mask"].float().reshape(B, -1, out["mask"].shape[-2], out["mask"].shape[-1])[:, 0, 0, :].cpu().numpy()
    names, sheets = CP.pitch_sheets(B, K, [float(a) for a in alphas], T, 512 / 16000, sx=sx, plot_height=PH)
    assert [n for _, n in names] == [p.name for p in paths]

    def markers(i):
        gap = np.flatnonzero(mask[i] == 0)
        return [(int(f) * c["hop"] + 256) // 512 for f in (gap[0], gap[-1] + 1)] if gap.size else [-1, -1]

    for p, (i, _), s in zip(paths, names, sheets):
        m = markers(i)
        im = Image.open(p)
        ref = R.render(values, s, (0, T, m[0], m[1]))
        assert im.mode == "P" and im.size == (ref.shape[1], ref.shape[0]), p
        assert bytes(im.getpalette()[:768]) == CP.plot_palette().tobytes()
        if p.name in ("pc_2_pitch.png", "pitch_comparison.png"):
            assert np.array_equal(np.asarray(im), ref), (p, np.argwhere(np.asarray(im) != ref)[:5].tolist())
    assert Image.open(paths[-1]).size[1] == (1 + K) * (4 + PH + 2 + 9)
    # the device call and the host renderer write the same files; fewer directions, no individual figures
    host = V.save_pc_pitch_plots(out, tmp_path / "host", alphas, first_index=4, sx=sx, plot_height=PH, hop_length=c["hop"], backend="host")
    assert [q.read_bytes() for q in host] == [p.read_bytes() for p in paths]
    only = V.save_pc_pitch_plots(out, tmp_path / "only", alphas, max_dirs=1, individual=False)
    assert [q.name for q in only] == ["pitch_comparison.png"] * B
    assert Image.open(only[0]).size[1] == 2 * (4 + 240 + 2 + 9)
    hop = out["clean_audio"].shape[-1] // (mask.shape[1] - 1)                  # the default STFT hop
    assert hop == c["hop"]
    sheet = CP.pitch_sheets(B, 1, [float(a) for a in alphas], T, 512 / 16000, individual=False, per_item=1 + K * A)[1][0]
    assert np.array_equal(np.asarray(Image.open(only[0])), R.render(values, sheet, (0, T, *markers(0))))


def test_audio_validator_writes_the_pitch_figures(tmp_path):
    from golden_util import load
    from nppc_audio import curve_png as CP
    from nppc_audio import validator as AV
    _, meta = load("g1_c1")
    c = meta["config"]
    spec = W.nppc_spec(c["K"], num_freqs=c["F"], sb_neighbors=c["sbn"], sb_hidden=c["sbh"])
    wts = {k: torch.from_numpy(v) for k, v in W.make_weights(spec, c["seed"]).items()}
    pre = "pretrained_restoration_model."
    ck = os.path.join(str(tmp_path), "restorer.tar")
    torch.save({"model": {k[len(pre):]: v for k, v in wts.items() if k.startswith(pre)}}, ck)
    common = dict(num_freqs=c["F"], sb_num_neighbors=c["sbn"], sb_model_hidden_size=c["sbh"], precision="fp32")
    model_cfg = dict(
        pretrained_restoration_model_configuration=dict(common, num_groups_in_drop_band=c["G_rest"]),
        pretrained_restoration_model_path=ck,
        audio_pc_wrapper_configuration=dict(multi_direction_configuration=dict(common, num_groups_in_drop_band=c["G_pc"],
                                                                               n_directions=c["K"])),
        stft_configuration=dict(nfft=c["nfft"], hop_length=c["hop"], win_length=c["nfft"]), device="cuda")
    nppc = os.path.join(str(tmp_path), "nppc.pt")
    torch.save({"model_state_dict": wts, "step": 0}, nppc)
    val = AV.NPPCAudioValidator(AV.NPPCAudioValidatorConfig(nppc_audio_model_configuration=model_cfg, checkpoint_path=nppc))
    noisy = torch.from_numpy(W.synth_batch(1, 8192)[0])
    paths, pitch = val.visualize_pc_pitch(noisy, save_dir=tmp_path / "se", sx=4, plot_height=40)
    K, T = c["K"], 1 + 8192 // 512
    assert [str(p) for p in paths] == [str(tmp_path / "se" / "pitch" / f"pc_{k}_pitch.png") for k in range(1, K + 1)] + \
        [str(tmp_path / "se" / "pitch" / "pitch_comparison.png")]
    values = CP.stack_contours(pitch).cpu().numpy()
    names, sheets = CP.pitch_sheets(1, K, list(AV.ALPHAS), T, 512 / 16000, sx=4, plot_height=40, markers=False)
    for p, s in zip(paths, sheets):
        assert np.array_equal(np.asarray(Image.open(p)), R.render(values, s, (0, T, -1, -1))), p
    with pytest.raises(ValueError, match="save_dir"):
        val.visualize_pc_pitch(noisy)
