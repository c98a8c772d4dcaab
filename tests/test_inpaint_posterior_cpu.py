"""CPU: the posterior samples of inpainted gaps -- the restatement (tests/inpaint_posterior_ref.py)
at its anchors, every refusal that needs no GPU, the tiling rule of nppc_inp_post_sample_shape and the error codes of the new
entry points."""
import ctypes

import pytest
import torch

import inpaint_posterior_ref as PR
import inpaint_validator_ref as VR


def IP():
    from nppc_audio.inpainting import posterior
    return posterior


def inputs(B, K, n_fft, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    F = n_fft // 2 + 1
    pred = (torch.rand(B, 1, F, T, generator=g) * 2 - 1) * 2.0
    pc = (torch.rand(B, K, F, T, generator=g) * 2 - 1) * 0.6
    clean_spec = torch.randn(B, 2, F, T, generator=g) * (torch.rand(B, 1, F, T, generator=g) >= 0.05)
    return pred, pc, clean_spec, torch.tensor(-1.0), torch.tensor(2.5)


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n_fft,hop,T,K", [(255, 128, 9, 3), (100, 25, 12, 1)])
def test_restatement_at_one_hot_coefficients_is_the_pc_variation_chain(n_fft, hop, T, K, dtype):
    B = 2
    pred, pc, clean_spec, mean, std = inputs(B, K, n_fft, T)
    alphas = torch.arange(-3, 3.5, 0.5)
    z = PR.one_hot_coefficients(B, K, alphas)
    assert z.shape == (B, K * 13, K) and float(z[1, 13 * (K - 1) + 2, K - 1]) == -2.0 and int((z != 0).sum()) == B * K * 12
    got = PR.sample_waveforms(pred, pc, clean_spec, z, mean, std, n_fft, hop, dtype)
    want, _ = VR.pc_variation_chain(pred, pred, pc, clean_spec, alphas, mean, std, n_fft, hop, dtype)
    assert got.dtype == dtype and torch.equal(got.view(B, K, 13, -1), want)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_at_zero_coefficients_is_the_prediction(dtype):
    B, K, n_fft, hop, T = 2, 4, 254, 127, 7
    pred, pc, clean_spec, mean, std = inputs(B, K, n_fft, T, seed=3)
    got = PR.sample_waveforms(pred, pc, clean_spec, torch.zeros(B, 2, K), mean, std, n_fft, hop, dtype)
    want, _ = VR.pc_variation_chain(pred, pred, pc[:, :1], clean_spec, torch.zeros(1), mean, std, n_fft, hop, dtype)
    assert torch.equal(got[:, 0], want[:, 0, 0]) and torch.equal(got[:, 1], want[:, 0, 0])
    mag = PR.sample_magnitudes(pred, pc, torch.zeros(B, 1, K), mean, std, dtype)
    assert torch.equal(mag[:, 0], torch.exp(pred[:, 0].to(dtype) * std.to(dtype) + mean.to(dtype)))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_check_sample_args_refuses_from_shapes_alone():
    P = IP()
    F, T, B, K, S = 128, 9, 2, 5, 4
    ok = dict(pred_shape=(B, 1, F, T), pc_shape=(B, K, F, T), clean_shape=(B, 2, F, T), z_shape=(B, S, K), n_fft=255,
              hop_length=128, length=None, samples=True, stats=False, spec_stats=False)
    assert P.check_sample_args(**ok) == (B, S, K, F, T, 1025)
    assert P.check_sample_args(**{**ok, "stats": True, "spec_stats": True, "samples": False, "length": 700})[-1] == 700
    bad = [({"samples": False}, "nothing asked for"),
           ({"n_fft": 1023, "pc_shape": (B, K, 512, T), "pred_shape": (B, 1, 512, T), "clean_shape": (B, 2, 512, T)}, "> 512"),
           ({"n_fft": 256}, "do not fit n_fft"),
           ({"hop_length": 16}, "ceil"),
           ({"hop_length": 0}, "hop"),
           ({"hop_length": 255}, "window overlap add min"),
           ({"pc_shape": (B, 17, F, T), "z_shape": (B, S, 17)}, "at most 16"),
           ({"pc_shape": (B, F, T)}, r"\[B,K,F,T\]"),
           ({"pred_shape": (B, F, T)}, "pred_spec_mag"),
           ({"clean_shape": (B, 1, F, T)}, "clean_spec"),
           ({"z_shape": (B, S, K, 2)}, "coefficients"),
           ({"z_shape": (B, 0, K)}, "S >= 1"),
           ({"z_shape": (B + 1, S, K)}, "coefficients"),
           ({"z_shape": (B, S, K + 1)}, "coefficients"),
           ({"z_shape": (B, 1, K), "stats": True}, "2 <= S <= 4096"),
           ({"z_shape": (B, 4097, K), "spec_stats": True}, "2 <= S <= 4096"),
           ({"length": 0}, "no samples")]
    for change, match in bad:
        with pytest.raises(ValueError, match=match):
            P.check_sample_args(**{**ok, **change})
    with pytest.raises(ValueError, match="complex"):
        P.as_coefficients(torch.zeros(B, S, K, dtype=torch.complex64))
    with pytest.raises(ValueError, match=r"\[B,S,K\]"):
        P.as_coefficients(torch.zeros(B, S, K, 2))
    with pytest.raises(ValueError, match="tensor"):
        P.as_coefficients([[0.0]])
    # the two public calls refuse before they need a GPU
    pred, pc, clean_spec, mean, std = inputs(B, K, 255, T)
    with pytest.raises(ValueError, match="complex"):
        P.sample_waveforms(pred, pc, clean_spec, torch.zeros(B, S, K, dtype=torch.complex64), mean, std)
    with pytest.raises(ValueError, match="2 <= S"):
        P.sample_waveforms(pred, pc, clean_spec, torch.zeros(B, 1, K), mean, std, stats=True)
    with pytest.raises(ValueError, match="coefficients"):
        P.sample_waveforms_blind(pred, pc, clean_spec, torch.ones(B, T), torch.zeros(B, S, K + 1), mean, std)
    with pytest.raises(ValueError, match="complex"):
        P.sample_waveforms_blind(pred, pc, clean_spec, torch.ones(B, T), torch.zeros(B, S, K, dtype=torch.complex64), mean, std)


def test_sampler_refuses_clean_phase_without_the_clean_spectrum():
    P = IP()
    s = P.InpaintingPosteriorSampler(model=torch.nn.Linear(1, 1))
    with pytest.raises(ValueError, match="clean_spec"):
        s.sample(torch.zeros(1, 2, 128, 9), torch.ones(1, 9))
    with pytest.raises(ValueError, match="phase"):
        s.sample(torch.zeros(1, 2, 128, 9), torch.ones(1, 9), phase="random")


# ---- the shape query --------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 5, 9, 255, 128), (1, 64, 5, 500, 255, 128), (16, 256, 5, 500, 255, 128), (2, 17, 16, 37, 255, 128),
          (2, 17, 16, 9, 512, 256), (2, 9, 16, 41, 100, 25), (2, 9, 5, 41, 100, 25), (3, 4096, 1, 9, 254, 127), (1, 2, 0, 3, 64, 16)]


@pytest.mark.parametrize("B,S,K,T,n_fft,hop", SHAPES)
def test_shape_query_against_its_restatement(B, S, K, T, n_fft, hop):
    P = IP()
    L = hop * (T - 1) + (n_fft & 1)
    for length in (L, L + 300, max(1, L - 100)):
        for stats in (0, 1, 2, 3):
            if stats and S < 2:
                continue
            for no_stage in (False, True):
                got = P.sample_shape(B, S, K, T, n_fft, hop, length, stats, no_stage)
                want = PR.tiling(B, S, K, T, n_fft, hop, length, stats, no_stage)
                assert (got["tiles"], got["tile_samples"], got["work_bytes"], int(got["staged"]), got["lds_bytes"]) == want
                assert got["tiles"] * got["tile_samples"] >= S > (got["tiles"] - 1) * got["tile_samples"]
                assert got["lds_bytes"] <= 65536 and got["length"] == length and not (no_stage and got["staged"])


def test_shape_query_paths_and_refusals():
    P = IP()
    # the validator's shape is staged; 16 directions at 512 / 256 and at 100 / 25 are not; B = 1 without statistics still
    # gets ceil(S / 8) tiles, with statistics only as many as fill the chip
    assert P.sample_shape(16, 64, 5, 500)["staged"] and P.sample_shape(2, 4, 16, 37)["staged"]
    assert not P.sample_shape(2, 4, 16, 9, 512, 256)["staged"] and not P.sample_shape(2, 4, 16, 41, 100, 25)["staged"]
    assert P.sample_shape(1, 256, 5, 500)["tiles"] == 32 and P.sample_shape(1, 256, 5, 500, stats=1)["tiles"] == 5
    assert P.sample_shape(16, 256, 5, 500, stats=3)["tiles"] == 1
    for kw in (dict(S=0), dict(K=17), dict(K=-1), dict(B=0), dict(B=65536), dict(n_fft=1023, hop_length=512), dict(hop_length=16),
               dict(S=1, stats=1), dict(S=4097, stats=2), dict(stats=4), dict(length=0), dict(T=0)):
        args = {**dict(B=2, S=4, K=5, T=9), **kw}
        with pytest.raises(ValueError):
            P.sample_shape(**args)
    with pytest.raises(ValueError, match="window overlap add min"):
        P.sample_shape(1, 2, 1, 4, 100, 100)


# ---- error codes of the entry points ----------------------------------------------------------------------------------------
def test_entry_points_refuse_null_pointers_and_bad_arguments_before_any_launch():
    from nppc_audio import _hip as H
    host = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(host))                 # non-null; a refused call never reads it
    B, S, K, T, N, hop, L = 1, 2, 3, 9, 255, 128, 1025

    def sample(ptrs=None, **kw):
        a = dict(pred=p, pc=p, clean=p, mean=p, sd=p, z=p, B=B, S=S, K=K, T=T, N=N, hop=hop, L=L, flags=0, samples=p, m=None,
                 s=None, mm=None, ms=None, work=None, wb=0)
        a.update(kw)
        H.call("nppc_inp_post_sample", *a.values(), None)

    for kw in (dict(pred=None), dict(pc=None), dict(clean=None), dict(mean=None), dict(sd=None), dict(z=None),
               dict(samples=None),                                               # nothing asked for
               dict(m=p), dict(s=p), dict(mm=p), dict(ms=p),                     # a mean without its std and the like
               dict(m=p, s=p), dict(m=p, s=p, work=p, wb=8),                     # statistics without (enough) workspace
               dict(m=p, s=p, S=1, work=p, wb=1 << 20), dict(m=p, s=p, S=4097, work=p, wb=1 << 30),
               dict(K=17), dict(S=0), dict(N=1023, hop=512), dict(hop=16), dict(hop=255), dict(flags=2), dict(B=0), dict(L=0)):
        with pytest.raises(RuntimeError, match="bad argument"):
            sample(**kw)

    def blind(name, tail, **kw):
        a = dict(pred=p, pc=p, mean=p, sd=p, z=p, known=p, mask=p, phase=p, out=p, dist=p, tn=p, status=p, work=p, wb=1 << 30,
                 B=B, K=K, S=S, T=T, N=N, hop=hop, L=L, n_iter=2, mom=0.0, max_span=0)
        a.update(kw)
        H.call(name, *a.values(), *tail, None)

    for name, tail in (("nppc_gl_gap_post", ()), ("nppc_gl_gap_post_long", (0, 1))):
        for kw in (dict(pred=None), dict(pc=None), dict(mean=None), dict(sd=None), dict(z=None), dict(known=None), dict(mask=None),
                   dict(phase=None), dict(out=None), dict(status=None), dict(work=None), dict(K=0), dict(K=17), dict(S=0),
                   dict(S=65535), dict(wb=8), dict(n_iter=-1)):
            with pytest.raises(RuntimeError, match="bad argument"):
                blind(name, tail, **kw)
    with pytest.raises(RuntimeError, match="bad argument"):
        blind("nppc_gl_gap_post_long", (0, 3))                                   # mode is 1 or 2


# ---- coefficients -----------------------------------------------------------------------------------------------------------
def test_a_seed_means_the_same_coefficients_as_the_speech_enhancement_sampler():
    from nppc_audio import posterior as SE
    P = IP()
    z = P.draw_coefficients(3, 7, 5, seed=11, device="cpu")
    ref = SE.draw_coefficients(3, 7, 5, seed=11, device="cpu")
    assert z.shape == (3, 7, 5) and z.dtype == torch.float32 and z.is_contiguous() and torch.equal(z, ref[..., 0])
    assert torch.equal(P.draw_coefficients(3, 7, 5, seed=11, temperature=0.5, device="cpu"),
                       SE.draw_coefficients(3, 7, 5, seed=11, temperature=0.5, device="cpu")[..., 0])
    g = torch.Generator().manual_seed(4)
    assert torch.equal(P.draw_coefficients(2, 3, 4, generator=g, device="cpu"),
                       SE.draw_coefficients(2, 3, 4, generator=torch.Generator().manual_seed(4), device="cpu")[..., 0])
    with pytest.raises(ValueError):
        P.draw_coefficients(2, 0, 4, device="cpu")


# ---- whole recordings -------------------------------------------------------------------------------------------------------
def test_restore_refuses_bad_sample_arguments_without_a_gpu():
    from test_restore_cpu import model_configuration
    from nppc_audio.inpainting.restore import RecordingRestorer, RecordingRestorerConfig
    r = RecordingRestorer.__new__(RecordingRestorer)                                    # no checkpoint, no model, no device
    r.config = RecordingRestorerConfig(checkpoint_path="x", model_configuration=model_configuration())
    r.device = "cpu"
    K = r.config.model_configuration.audio_pc_wrapper_configuration.n_dirs
    x, gaps = torch.randn(40000), [(20000, 21000)]
    for bad in (0, -2, 2.5, True):
        with pytest.raises(ValueError, match="samples"):
            r.restore(x, gaps, samples=bad)
        with pytest.raises(ValueError, match="samples"):
            r.restore(x, gaps, samples=bad, sample_rate=44100)
    for shape in ((2, 3, K), (1, 3, K + 1), (1, 0, K), (3, K), (1, 3, K, 2)):
        with pytest.raises(ValueError, match="coeffs"):
            r.restore(x, gaps, coeffs=torch.zeros(shape))
    with pytest.raises(ValueError, match="coeffs"):
        r.restore(x, gaps, samples=4, coeffs=torch.zeros(1, 3, K))
    with pytest.raises(ValueError, match="complex"):
        r.restore(x, gaps, coeffs=torch.zeros(1, 3, K, dtype=torch.complex64))
    out = r.restore(torch.randn(1000), [], samples=3)                                   # no gaps: nothing to sample
    assert out["windows"] == [] and out["sample_windows"] is None and out["coeffs"] is None
    assert set(r.restore(torch.randn(1000), [])) == {"restored", "windows", "gain", "inconsistency", "target_norm", "status"}
