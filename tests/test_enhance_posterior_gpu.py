"""GPU: posterior samples of whole recordings (csrc/enhance_post.hip, enhance.sample_chunks, RecordingEnhancer.enhance(samples=);
DESIGN.md section 7j) against the fp64 restatement (tests/enhance_posterior_ref.py) and against the composed path of the
functions that were there before: w_mat gathered to slot order with torch, posterior.sample_waveforms on the chunks, then
enhance.splice per sample row.

Kernel-level shapes: synthetic planes of posterior_ref.case with the chunks as the batch; (n_fft, hop) every entry of
test_posterior_gpu.CONFIGS (all have 2 <= n_fft / hop <= 8); K in {1, 5, 16}; S in {1, 3, TILE + 1}; per (configuration, K, S)
the plans PLANS: n in {1, 2, 5}, half a chunk of 1, 2 and 8 output blocks of 4 hop samples, last chunks of H + 1, C - 1 and C
samples and one chunk shorter than C.

1. closeness: fused and composed errors against the restatement, max-abs and RMS over the peak; fused <= 4 x composed (both
   are fp32 evaluations of one formula; test_posterior_gpu's convention and margin).  Bit-equality is recorded, not asserted.
2. z = 0 is enhance(wave)["enhanced"], bit for bit, in both domains.
3. a signed permutation of the raw directions with recomputed tables changes no bit; with identity tables it does.
4. run, S and stats-only independence, statistics against fp64 of the returned samples, the padding of the rows untouched.
5. RecordingEnhancer end to end on the small model of test_enhance_gpu."""
import json
import os

import numpy as np
import pytest
import torch

import enhance_posterior_ref as EP
import enhance_ref as ER
from nppc_validation_ref import clips
from test_enhance_gpu import CHUNK, bits, by_hand, enhancer  # noqa: F401  (enhancer: the module-scoped fixture)
from test_posterior_gpu import CONFIGS, errors

pytestmark = pytest.mark.gpu
_RECORD = {}
# (n, output blocks in half a chunk, the last chunk as a function of C)
PLANS = [(1, 2, lambda C: C - 37), (2, 1, lambda C: C // 2 + 1), (5, 2, lambda C: C - 1), (2, 8, lambda C: C)]


@pytest.fixture(scope="module", autouse=True)
def parity_file():
    """NPPC_ENHANCE_POSTERIOR_PARITY_OUT=<file>: the errors of both paths and whether they were bit-equal, per case, as JSON
    (profiles/enhance_posterior_parity_errors.json is such a run)"""
    yield
    path = os.environ.get("NPPC_ENHANCE_POSTERIOR_PARITY_OUT")
    if _RECORD and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump(_RECORD, open(path, "w"), indent=1, sort_keys=True)


def E():
    from nppc_audio import enhance
    return enhance


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def tables(n, K, seed):
    """any tables are an input the kernel has to follow: a random permutation and random signs per chunk"""
    rng = np.random.default_rng(seed)
    perm = np.stack([rng.permutation(K) for _ in range(n)]).astype(np.int32)
    return perm, rng.choice([-1, 1], (n, K)).astype(np.int32)


def fused(case, perm, sign, last, C, nfft, hop, **kw):
    pred, w, re, im, z = case
    return E().sample_chunks(dev(pred), dev(w), dev(re), dev(im), None, dev(z), dev(perm), dev(sign), last, C, nfft, hop, **kw)


def composed(case, perm, sign, last, C, nfft, hop, domain="compressed"):
    """the parent's functions: gather with torch, the clip sampler on the chunks ([n, S, C]), one splice per sample -> [S, L]"""
    from nppc_audio import posterior as P
    pred, w, re, im, z = (dev(a) for a in case)
    n, S = pred.shape[0], z.shape[0]
    W = C if n > 1 else last
    slot = w[torch.arange(n, device="cuda")[:, None], dev(perm).long()] * dev(sign).float()[:, :, None, None, None]
    y = P.sample_waveforms(pred, slot, re, im, z[None].expand(n, *z.shape), W, nfft, hop, lengths=EP.chunk_lengths(n, C, last),
                           domain=domain)["samples"]
    buf = torch.zeros(n, S, C, device="cuda")
    buf[:, :, :W] = y
    return torch.stack([E().splice(buf[:, s], None, last, None, None, None)[0] for s in range(S)])


@pytest.mark.parametrize("S", [1, 3, 9])
@pytest.mark.parametrize("K", [1, 5, 16])
@pytest.mark.parametrize("nfft,hop", CONFIGS)
def test_fused_launch_is_as_close_to_fp64_as_the_composed_path(nfft, hop, K, S):
    from nppc_audio import posterior as P
    assert S in (1, 3, P.TILE + 1)
    for p, (n, blocks, last_of) in enumerate(PLANS):
        C = 2 * blocks * 4 * hop
        last = last_of(C)
        L = (n - 1) * (C // 2) + last
        assert EP.shape_ok(n, S, K, C, L, 1 + (C if n > 1 else last) // hop, nfft, hop) and last > nfft // 2
        case = EP.case(n, S, K, C, last, nfft, hop, seed=1000 * K + 10 * S + p, complex_coeffs=p != 0)
        perm, sign = tables(n, K, seed=p + K)
        for domain in ("compressed", "decompressed"):
            tag = f"n{nfft}_h{hop}_K{K}_S{S}_chunks{n}_C{C}_last{last}_{domain}"
            want = EP.sample_recording(*case, perm, sign, last, C, nfft, hop, domain)
            f = fused(case, perm, sign, last, C, nfft, hop, domain=domain)["samples"]
            c = composed(case, perm, sign, last, C, nfft, hop, domain)
            assert tuple(f.shape) == (S, L) == tuple(c.shape)
            fe, ce = errors(f, want), errors(c, want)
            _RECORD[tag] = dict(fused_maxabs=fe[0], fused_rms=fe[1], composed_maxabs=ce[0], composed_rms=ce[1],
                                bit_equal=bool(torch.equal(f, c)))
            print(f"{tag}: fused {fe[0]:.3e} / {fe[1]:.3e}, composed {ce[0]:.3e} / {ce[1]:.3e}, bit-equal {_RECORD[tag]['bit_equal']}")
            assert fe[0] <= 4 * ce[0] and fe[1] <= 4 * ce[1], (tag, fe, ce)


# ---- the alignment -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,C,n,nfft,hop", [(5, 256, 3, 64, 16), (16, 128, 5, 64, 8), (3, 4096, 2, 512, 256)])
def test_signed_permutations_of_the_raw_directions_change_nothing_but_only_with_recomputed_tables(K, C, n, nfft, hop):
    """direction waveforms of enhance_ref.directions (cosines far from ties) give the tables, before and after the same signed
    permutation moves them and the planes of every chunk but the first"""
    en = E()
    S, last = 9, C - 3
    _, pcs, tp, ts = ER.directions(K, C, n, seed=2)
    rp, rs, _, gap = ER.chain(pcs)
    assert gap >= 0.1 and np.array_equal(rp, tp) and np.array_equal(rs, ts)      # before anything is compared: no near-tie
    perms, signs = ER.signed_permutations(np.random.default_rng(1), n, K)
    assert not np.array_equal(perms, np.tile(np.arange(K), (n, 1))) or K == 1
    case = EP.case(n, S, K, C, last, nfft, hop, seed=9, complex_coeffs=True)
    moved_case = (case[0], ER.apply_signed(case[1].reshape(n, K, -1), perms, signs).reshape(case[1].shape)) + case[2:]

    def run(cs, p):
        perm, sign, _ = en.chain(en.boundary_gram(dev(p))[0], n, K)
        pred, w, re, im, z = (dev(a) for a in cs)
        return [en.sample_chunks(pred, w, re, im, None, z, perm, sign, last, C, nfft, hop, domain=d, stats=True)
                for d in ("compressed", "decompressed")], perm, sign

    base, perm, sign = run(case, pcs)
    again, mperm, msign = run(moved_case, ER.apply_signed(pcs, perms, signs))
    assert np.array_equal(perm.cpu().numpy(), rp) and np.array_equal(sign.cpu().numpy(), rs)
    want = EP.moved_tables(rp, rs, perms, signs)
    assert np.array_equal(mperm.cpu().numpy(), want[0]) and np.array_equal(msign.cpu().numpy(), want[1])
    for a, b in zip(base, again):
        for key in ("samples", "mean", "std"):
            assert np.array_equal(bits(a[key]), bits(b[key])), key
    # the fault itself: the same two inputs with perm = identity and sign = +1 differ
    ident = np.tile(np.arange(K, dtype=np.int32), (n, 1))
    plain = [fused(cs, ident, np.ones_like(ident), last, C, nfft, hop)["samples"] for cs in (case, moved_case)]
    assert not np.array_equal(bits(plain[0]), bits(plain[1]))


# ---- exact properties of the launch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,hop,n,blocks,S", [(64, 8, 5, 1, 9), (64, 32, 2, 2, 40), (512, 256, 3, 1, 9), (64, 16, 1, 2, 2)])
def test_run_sample_and_statistics_independence(nfft, hop, n, blocks, S):
    from nppc_audio import _hip as H
    K = 5
    C = 2 * blocks * 4 * hop
    last = C - 5
    L = (n - 1) * (C // 2) + last
    case = EP.case(n, S, K, C, last, nfft, hop, seed=21 + S, complex_coeffs=True)
    perm, sign = tables(n, K, seed=S)
    a = fused(case, perm, sign, last, C, nfft, hop, stats=True)
    b = fused(case, perm, sign, last, C, nfft, hop, stats=True)
    only = fused(case, perm, sign, last, C, nfft, hop, samples=False, stats=True)
    assert "samples" not in only and tuple(a["samples"].shape) == (S, L) and tuple(a["mean"].shape) == (L,)
    for key in ("samples", "mean", "std"):
        assert torch.equal(a[key], b[key]), key                     # run to run
    for key in ("mean", "std"):
        assert torch.equal(a[key], only[key]), key                  # stats-only == stats of a call that returns samples
    for s in sorted({0, S // 2, S - 1}):                            # a sample alone; the last lies behind a tile boundary
        one = fused(case[:4] + (case[4][s:s + 1],), perm, sign, last, C, nfft, hop)["samples"]
        assert torch.equal(one[0], a["samples"][s]), s
    # mean / std: the fp64 mean and unbiased deviation of the returned samples, rounded to fp32.  The launch sums y and y^2
    # in fp64 (one pass); against the two-pass value that costs a cancellation of at most sqrt(S 2^-52) peak, far below
    # half an fp32 ulp of the value except where the deviation itself is tiny: the bounds of test_posterior_gpu.
    y = a["samples"].double().cpu().numpy()
    m = y.mean(axis=0)
    sd = np.sqrt(((y - m) ** 2).sum(axis=0) / (S - 1))
    peak = np.abs(y).max()
    em = np.abs(a["mean"].double().cpu().numpy() - m).max() / peak
    es = np.abs(a["std"].double().cpu().numpy() - sd).max() / peak
    print(f"n{nfft} h{hop} S{S}: mean {em:.3e}, std {es:.3e}")
    assert em <= 1.2e-7 and es <= 1e-6, (em, es)
    # and exactly the fp64 one-pass values of the returned samples, rounded to fp32 once
    tiles, per, _ = EP.tiling(S, L, hop, stats=1)
    mean32, std32 = EP.one_pass_stats(a["samples"].cpu().numpy(), tiles, per)
    assert np.array_equal(bits(a["mean"]), bits(mean32)) and np.array_equal(bits(a["std"]), bits(std32))
    # rows with padding: nothing past L is written
    pred, w, re, im, z = (dev(x) for x in case)
    ldo = L + 7
    store = torch.full((S, ldo), float("nan"), device="cuda")
    poison = bits(store).copy()
    H.call("nppc_enh_post_sample", pred, w, re, im, z, dev(perm), dev(sign), E().hann_table(C, "cuda") if n > 1 else None, 0, n, S,
           K, C, L, pred.shape[-1], nfft, hop, store, ldo, None, None, None, 0, H.stream())
    assert np.array_equal(bits(store[:, :L]), bits(a["samples"])) and np.array_equal(bits(store[:, L:]), poison[:, L:])


# ---- end to end ----------------------------------------------------------------------------------------------------------
RECORDING = 2603                           # 5 chunks of 1024 in 3 batches of 2, a last chunk of 555 samples


def planes_by_hand(enh, x):
    """pred_crm, w_mat, re, im of every chunk from NPPCModel's public pieces, batch by batch as enhance runs them"""
    from nppc_audio import ops
    model, c = enh.model, enh.config
    st = c.model_configuration.stft_configuration
    plan = ER.plan(x.numel(), CHUNK)
    n, W = len(plan), (x.numel() if len(plan) == 1 else CHUNK)
    chunks = torch.zeros(n, W, device="cuda")
    for i, (s, ln) in enumerate(plan):
        chunks[i, :ln] = x[s:s + ln]
    out = [[], [], [], []]
    with torch.no_grad():
        for b0 in range(0, n, c.chunk_batch):
            xb = chunks[b0:b0 + c.chunk_batch]
            lens = [ln for _, ln in plan[b0:b0 + c.chunk_batch]]
            w_mat = model(xb, lengths=lens)
            crm = model.get_pred_crm(xb, lengths=lens)
            _, re, im = ops.stft(xb, st.nfft, st.hop_length, want_mag=False, lengths=lens)
            for acc, t in zip(out, (crm, w_mat, re, im)):
                acc.append(t)
    return [torch.cat(a) for a in out], plan


def test_enhance_with_samples_is_sample_chunks_fed_by_hand(enhancer):
    from nppc_audio import posterior as P
    enh, c = enhancer
    st = enh.config.model_configuration.stft_configuration
    x = clips([RECORDING])[0][0].cuda()
    alphas = [-3.0, 1.0, 2.5]
    today_plain, today = by_hand(enh, x, None)[0], by_hand(enh, x, alphas)[0]
    plain, varied = enh.enhance(x), enh.enhance(x, alphas)
    assert set(plain) == {"enhanced", "chunks"} and np.array_equal(bits(plain["enhanced"]), bits(today_plain["enhanced"]))
    assert set(varied) == {"enhanced", "variations", "perm", "sign", "continuity", "chunks", "alphas"}
    for key in ("enhanced", "variations"):
        assert np.array_equal(bits(varied[key]), bits(today[key])), key
    for key in ("perm", "sign", "continuity"):
        assert torch.equal(varied[key], today[key]), key

    out = enh.enhance(x, samples=3, seed=4, stats=True)
    assert set(out) == {"enhanced", "chunks", "samples", "coeffs", "sample_mean", "sample_std", "perm", "sign", "continuity"}
    (pred, w_mat, re, im), plan = planes_by_hand(enh, x)
    assert out["chunks"] == plan and len(plan) == 5 and plan[-1] == (2048, 555)
    z = P.draw_coefficients(1, 3, c["K"], seed=4)[0]
    assert torch.equal(out["coeffs"], z)
    want = E().sample_chunks(pred, w_mat, re, im, [ln for _, ln in plan], z, varied["perm"], varied["sign"], 555, CHUNK, st.nfft,
                             st.hop_length, stats=True)
    assert tuple(out["samples"].shape) == (3, RECORDING) and np.array_equal(bits(out["samples"]), bits(want["samples"]))
    assert np.array_equal(bits(out["sample_mean"]), bits(want["mean"])) and np.array_equal(bits(out["sample_std"]), bits(want["std"]))
    for key in ("perm", "sign", "continuity"):                      # the tables are formed as with alphas
        assert torch.equal(out[key], varied[key]), key
    assert np.array_equal(bits(out["enhanced"]), bits(plain["enhanced"]))
    assert bool(torch.isfinite(out["samples"]).all()) and float(out["sample_std"].max()) > 0
    both = enh.enhance(x, alphas, samples=3, seed=4)                # with alphas: today's outputs and the same samples
    assert np.array_equal(bits(both["variations"]), bits(varied["variations"]))
    assert np.array_equal(bits(both["samples"]), bits(out["samples"])) and "sample_mean" not in both
    again = enh.enhance(x.cpu(), samples=3, seed=4)
    other = enh.enhance(x, samples=3, seed=5)
    assert np.array_equal(bits(again["samples"]), bits(out["samples"]))
    assert not np.array_equal(bits(other["samples"]), bits(out["samples"]))
    given = enh.enhance(x, coeffs=out["coeffs"][..., 0])            # real coefficients [S, K]
    assert np.array_equal(bits(given["samples"]), bits(out["samples"])) and torch.equal(given["coeffs"], out["coeffs"])
    stats_only = enh.enhance(x, samples=3, seed=4, keep_samples=False, stats=True)
    assert "samples" not in stats_only and torch.equal(stats_only["sample_mean"], out["sample_mean"])
    half = enh.enhance(x, samples=3, seed=4, temperature=0.5)
    assert torch.equal(half["coeffs"], P.draw_coefficients(1, 3, c["K"], seed=4, temperature=0.5)[0])
    with pytest.raises(ValueError, match="statistics need"):
        enh.enhance(x, samples=1, stats=True)
    with pytest.raises(ValueError, match="nothing asked"):
        enh.enhance(x, samples=2, keep_samples=False)
    with pytest.raises(ValueError, match="domain"):
        enh.enhance(x, samples=2, domain="linear")


@pytest.mark.parametrize("domain", ["compressed", "decompressed"])
def test_zero_coefficients_are_the_enhanced_recording_bit_for_bit(enhancer, domain):
    enh, c = enhancer
    for L, first in ((RECORDING, 179), (1001, 180), (1024 + 512, 181)):     # 5 chunks, one short chunk, two full chunks
        x = clips([L], first=first)[0][0].cuda()
        want = enh.enhance(x)["enhanced"]
        got = enh.enhance(x, coeffs=torch.zeros(2, c["K"]), domain=domain)["samples"]
        assert tuple(got.shape) == (2, L)
        for s in range(2):
            assert np.array_equal(bits(got[s]), bits(want)), (L, s, float((got[s] - want).abs().max()))


def test_samples_at_another_rate_are_down_enhance_up(enhancer):
    from nppc_audio import resample as RSM
    enh, c = enhancer
    N = 7001
    x = clips([N], first=185)[0][0].cuda()
    alphas = [-1.0, 2.0]
    out = enh.enhance(x, alphas, sample_rate=44100, samples=2, seed=3)
    low = RSM.resample(x, 44100, 16000, backend="hip")
    inner = enh.enhance(low, alphas, samples=2, seed=3)
    rows = torch.cat([inner["enhanced"][None], inner["variations"].reshape(-1, low.numel()), inner["samples"]]).contiguous()
    up = RSM.resample(rows, 16000, 44100, backend="hip")[:, :N]
    V = c["K"] * 2
    assert tuple(out["samples"].shape) == (2, N) and out["sample_rate"] == 44100 and len(inner["chunks"]) > 1
    assert np.array_equal(bits(out["enhanced"]), bits(up[0]))
    assert np.array_equal(bits(out["variations"]).reshape(-1, N), bits(up[1:1 + V]))
    assert np.array_equal(bits(out["samples"]), bits(up[1 + V:]))
    assert torch.equal(out["coeffs"], inner["coeffs"])
    with pytest.raises(ValueError, match="model's rate"):
        enh.enhance(x, sample_rate=44100, samples=2, stats=True)


def test_files_in_and_posterior_samples_out(enhancer, tmp_path):
    from scipy.io import wavfile
    from nppc_audio.flac import decode_files
    enh, c = enhancer
    x = clips([RECORDING])[0][0]
    pcm = np.clip(np.rint(x.numpy() / np.abs(x.numpy()).max() * 0.5 * 32768.0), -32768, 32767).astype(np.int16)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.flac")
    wavfile.write(src, 16000, pcm)
    out = enh.enhance_file(src, dst, samples=2, seed=1)
    direct = enh.enhance(torch.from_numpy(pcm.astype(np.float32) / 32768.0), samples=2, seed=1)
    assert np.array_equal(bits(out["samples"]), bits(direct["samples"])) and out["sample_rate"] == 16000
    paths = enh.save_posterior_samples(out, tmp_path / "p")
    assert [str(p) for p in paths] == [str(tmp_path / "p" / "posterior" / f"sample_{s}.flac") for s in range(2)]
    waves, infos = decode_files(paths, out="mono")
    for s in range(2):
        want = np.clip(np.rint(out["samples"][s].cpu().double().numpy() * 32768.0), -32768, 32767) / 32768.0
        assert infos[s].sample_rate == 16000 and np.array_equal(waves[s].cpu().numpy().astype(np.float64), want)
    assert not torch.equal(waves[0], waves[1])
    wavs = enh.save_posterior_samples(out, tmp_path / "w", fmt="wav")
    assert [os.path.basename(p) for p in wavs] == ["sample_0.wav", "sample_1.wav"] and all(os.path.getsize(p) > 44 for p in wavs)
    with pytest.raises(ValueError, match="no 'samples'"):
        enh.save_posterior_samples(enh.enhance(x), tmp_path / "q")
