"""The int8 encoder on the GPU: the quantiser kernels and the i8-MFMA GEMM bit
for bit against the numpy restatements of tests/test_int8_host.py, the int8 encoder against
the fp32 oracle with fake-quantised linear layers, mode switching, re-quantisation after
set_tensor, and the Python wiring (WhisperEngine / WhisperModel / JanusPipeline)."""
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from janus_amd import _native as nat
from janus_amd.whisper import CONFIGS, WhisperEngine, synthetic_weights
from janus_amd.workload import synth_speech
from oracle import packet as opk
from oracle import whisper as ow
from oracle.prosody import OracleProsody
from test_int8_host import dequant_np, exact_int_matmul, quant_rows_np

pytestmark = pytest.mark.gpu
EPI_F16, EPI_GELU_F16, EPI_RESID_F32, EPI_F32 = 0, 1, 2, 3


def stream():
    return torch.cuda.current_stream().cuda_stream


def edge_rows(K):
    """Zeros; the maximum carried by a negative element; ties at amax = 127; fp16 subnormals."""
    e = np.zeros((4, K), np.float16)
    e[1, :4] = [0.25, -3.0, 1.5, 2.5]
    e[2, :5] = [127.0, 0.5, 1.5, 2.5, -0.5]
    e[3] = (np.arange(K) % 7 - 3) * np.float16(2.0 ** -24)
    return e


# ---------------------------------------------------------------- 1. quant_rows_i8
@pytest.mark.parametrize("M,K,ldx", [(1, 384, 384), (37, 384, 400), (1, 2048, 2048), (37, 2048, 2048)])
def test_quant_rows_bit_exact(gpu, M, K, ldx):
    rng = np.random.default_rng(M * 31 + K)
    x = (rng.standard_normal((M, ldx)) * rng.uniform(0.01, 30.0, (M, 1))).astype(np.float16)
    if M >= 4:
        x[:4, :K] = edge_rows(K)
    else:
        x[0, :K] = edge_rows(K)[2]
    dx = torch.from_numpy(x).to(gpu)
    q = torch.full((M, K + 16), 99, dtype=torch.int8, device=gpu)
    s = torch.full((M,), -1.0, dtype=torch.float32, device=gpu)
    nat.call("janus_quant_rows_i8", dx.data_ptr(), ldx, q.data_ptr(), K + 16, s.data_ptr(), M, K, stream())
    torch.cuda.synchronize()
    rq, rs = quant_rows_np(x[:, :K])
    assert np.array_equal(q.cpu().numpy()[:, :K], rq)
    assert np.array_equal(s.cpu().numpy(), rs)
    assert (q.cpu().numpy()[:, K:] == 99).all()          # nothing written past K


# ---------------------------------------------------------- 2. layernorm_quant_i8
@pytest.mark.parametrize("d", [384, 512, 768])
def test_layernorm_quant_equals_two_passes(gpu, d):
    rows = 70
    g = torch.Generator().manual_seed(d)
    x = (torch.randn(rows, d, generator=g) * 3 + 0.5).to(gpu)
    x[5] = 0.0                                            # a constant row: LayerNorm gives beta
    gamma = (1 + 0.2 * torch.randn(d, generator=g)).to(gpu)
    beta = (0.1 * torch.randn(d, generator=g)).to(gpu)
    h = torch.empty(rows, d, dtype=torch.float16, device=gpu)
    q2 = torch.empty(rows, d, dtype=torch.int8, device=gpu)
    s2 = torch.empty(rows, dtype=torch.float32, device=gpu)
    nat.call("janus_layernorm_f16", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), h.data_ptr(),
             rows, d, 1e-5, stream())
    nat.call("janus_quant_rows_i8", h.data_ptr(), d, q2.data_ptr(), d, s2.data_ptr(), rows, d, stream())
    q1 = torch.empty(rows, d, dtype=torch.int8, device=gpu)
    s1 = torch.empty(rows, dtype=torch.float32, device=gpu)
    nat.call("janus_layernorm_quant_i8", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), q1.data_ptr(),
             s1.data_ptr(), rows, d, 1e-5, stream())
    torch.cuda.synchronize()
    assert torch.equal(q1, q2) and torch.equal(s1, s2)
    assert int(q1.abs().max()) == 127


# ------------------------------------------------------------------- 3. gemm_i8
SHAPES = [(1, 128, 128), (257, 256, 128), (255, 384, 384), (300, 1152, 384), (130, 768, 3072),
          (1500, 512, 2048)]


def run_gemm_i8(gpu, epi, A, W, sa, sw, bias, R=None):
    M, K = A.shape
    N = W.shape[0]
    dA, dW = torch.from_numpy(A).to(gpu), torch.from_numpy(W).to(gpu)
    dsa, dsw, db = (torch.from_numpy(v).to(gpu) for v in (sa, sw, bias))
    if epi == EPI_RESID_F32:
        C = torch.from_numpy(R).to(gpu).clone()           # R aliases C
    else:
        C = torch.empty(M, N, dtype=torch.float16 if epi in (EPI_F16, EPI_GELU_F16) else torch.float32,
                        device=gpu)
    nat.call("janus_gemm_i8", epi, dA.data_ptr(), K, dW.data_ptr(), K, dsa.data_ptr(), dsw.data_ptr(),
             db.data_ptr(), C.data_ptr(), N, C.data_ptr() if epi == EPI_RESID_F32 else None, N, M, N, K,
             stream())
    torch.cuda.synchronize()
    return C.cpu()


def check_gemm_i8(gpu, A, W, sa, sw, bias, R, epis=(EPI_F32, EPI_F16, EPI_RESID_F32, EPI_GELU_F16)):
    y = dequant_np(exact_int_matmul(A, W), sa, sw, bias)
    for epi in epis:
        got = run_gemm_i8(gpu, epi, A, W, sa, sw, bias, R)
        if epi == EPI_F32:
            assert np.array_equal(got.numpy(), y), epi
        elif epi == EPI_F16:
            assert np.array_equal(got.numpy(), y.astype(np.float16)), epi
        elif epi == EPI_RESID_F32:
            assert np.array_equal(got.numpy(), (R + y).astype(np.float32)), epi
        else:
            ref = F.gelu(torch.from_numpy(y).double())
            err = float((got.double() - ref).norm() / (ref.norm() + 1e-30))
            print(f"gelu rel err {err:.2e}")
            assert err < 2e-3, err


def scales(rng, M, N, K):
    # of the size the encoder has: activations of a few units, weights ~ 1 / sqrt(K)
    sa = (rng.uniform(0.5, 8.0, M) / 127).astype(np.float32)
    sw = (rng.uniform(0.5, 4.0, N) / np.sqrt(K) / 127).astype(np.float32)
    return sa, sw, rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_i8_full_range(gpu, M, N, K):
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    A = rng.integers(-127, 128, (M, K), dtype=np.int8)
    W = rng.integers(-127, 128, (N, K), dtype=np.int8)
    A[-1, 0], A[0, -1], W[-1, 0], W[0, -1] = -127, 127, 127, -127      # both extremes present
    assert A.min() == -127 and A.max() == 127 and W.min() == -127 and W.max() == 127
    check_gemm_i8(gpu, A, W, *scales(rng, M, N, K))


def test_gemm_i8_selector(gpu):
    """A = a 0/1 selector (row m picks k = (7 m + 3) % K), W asymmetric: C[m][n] = W[n][k(m)]
    exactly — a row/column swap or a mis-mapped fragment shows as wrong integers."""
    M, N, K = 300, 1152, 384
    A = np.zeros((M, K), np.int8)
    sel = (7 * np.arange(M) + 3) % K
    A[np.arange(M), sel] = 1
    W = ((3 * np.arange(N)[:, None] + 5 * np.arange(K)[None, :] ** 2) % 255 - 127).astype(np.int8)
    one_m, one_n = np.ones(M, np.float32), np.ones(N, np.float32)
    got = run_gemm_i8(gpu, EPI_F32, A, W, one_m, one_n, np.zeros(N, np.float32))
    assert np.array_equal(got.numpy(), W[:, sel].T.astype(np.float32))
    rng = np.random.default_rng(5)
    check_gemm_i8(gpu, A, W, *scales(rng, M, N, K), epis=(EPI_F32, EPI_RESID_F32))


def test_gemm_i8_all_127(gpu):
    """Every product 127 * 127 at K = 3072: the accumulator 49 548 288 is above 2^24 (nothing
    saturates, nothing goes through fp32 on the way); W rows with their first n % 7 elements
    at 126 give accumulators that are no multiple of the fp32 spacing 4 there, ties included
    (n % 7 == 2), so the int -> float conversion must round to nearest even."""
    M, N, K = 130, 768, 3072
    A = np.full((M, K), 127, np.int8)
    W = np.full((N, K), 127, np.int8)
    for n in range(N):
        W[n, :n % 7] = 126
    one_m, one_n, zero = np.ones(M, np.float32), np.ones(N, np.float32), np.zeros(N, np.float32)
    got = run_gemm_i8(gpu, EPI_F32, A, W, one_m, one_n, zero).numpy()
    acc = 49548288 - 127 * (np.arange(N) % 7)
    assert acc[0] > 2 ** 24 and (acc[2] % 4 == 2)
    assert np.array_equal(got, np.broadcast_to(acc.astype(np.float32), (M, N)))
    rng = np.random.default_rng(6)
    check_gemm_i8(gpu, A, W, *scales(rng, M, N, K), epis=(EPI_F32, EPI_F16, EPI_RESID_F32))


@pytest.mark.parametrize("M,N,K", [(64, 192, 128), (64, 128, 192), (64, 130, 128), (64, 128, 64)])
def test_gemm_i8_rejects_other_shapes(gpu, M, N, K):
    A = torch.zeros(M, K, dtype=torch.int8, device=gpu)
    W = torch.zeros(N, K, dtype=torch.int8, device=gpu)
    s = torch.ones(max(M, N), device=gpu)
    C = torch.zeros(M, N, device=gpu)
    with pytest.raises(nat.JanusNativeError):
        nat.call("janus_gemm_i8", EPI_F32, A.data_ptr(), K, W.data_ptr(), K, s.data_ptr(), s.data_ptr(),
                 s.data_ptr(), C.data_ptr(), N, None, N, M, N, K, stream())


# ------------------------------------------------------- 4. encoder against the oracle
def fake_quant_lin(x, W, p, bias=True):
    """oracle.whisper._lin with the encoder layers' linears fake-quantised: weight rows and
    activation rows through the row-wise quantiser, the integer product exact, then
    float(acc) * (sx * sw) + bias."""
    if not p.startswith("encoder.layers."):
        return real_lin(x, W, p, bias)
    wq, ws = quant_rows_np(np.asarray(W[p + ".weight"], np.float32))
    xq, xs = quant_rows_np(x.numpy())
    acc = torch.from_numpy(xq.astype(np.float64)) @ torch.from_numpy(wq.astype(np.float64)).T
    y = acc * (torch.from_numpy(xs.astype(np.float64))[..., None] * torch.from_numpy(ws.astype(np.float64)))
    if bias and (p + ".bias") in W:
        y = y + torch.from_numpy(np.asarray(W[p + ".bias"], np.float64))
    return y.float()


real_lin = ow._lin


def rel_rms(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def pack(utts, dev):
    lengths = [len(u) for u in utts]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    pcm = torch.from_numpy(np.concatenate(utts + [np.zeros(1, np.float32)])).to(dev)
    return pcm, offs


@pytest.fixture(scope="module")
def tiny(gpu):
    """tiny.en, seed 5: an int8 engine, an fp16 engine, the weights, the mel of one 30 s and
    one 9 s clip (B * 1500 = 3000 rows: no multiple of the GEMM's 128-row tile)."""
    cfg = CONFIGS["tiny.en"]
    W = synthetic_weights(cfg, seed=5)
    e8 = WhisperEngine(cfg, W, encoder_compute="int8")
    e16 = WhisperEngine(cfg, W)
    pcm, offs = pack([synth_speech(30, 30.0), synth_speech(31, 9.0)], gpu)
    mel = e16.logmel(pcm, offs, 2, 3)
    torch.cuda.synchronize()
    return cfg, W, e8, e16, mel


def encoder_against_oracle(cfg, W, e8, e16, mel, name):
    """The assertions of the int8 encoder test. The bound: the oracle with activations
    rounded to fp16 ahead of the quantiser (what the GPU path does) lies at 1.00 e_q from the
    fp32 oracle (tiny.en seed 5: e_q 1.94e-2, base.en seed 5: 2.27e-2, on the CPU); 1.25 e_q
    leaves room for the fp16 attention and GEMM outputs (4e-4 today), and a wrong scale or
    fragment map gives an error of order 1."""
    assert e8.encoder_compute == "int8" and e16.encoder_compute == "float16"
    g8 = e8.encode(mel).float().cpu()
    g16 = e16.encode(mel).float().cpu()
    torch.cuda.synchronize()
    m = mel.float().cpu().numpy()
    ref = ow.encoder(m, W, cfg)
    with mock.patch.object(ow, "_lin", fake_quant_lin):
        fq = ow.encoder(m, W, cfg)
    e_q = rel_rms(fq, ref)
    r8, r16, r816 = rel_rms(g8, ref), rel_rms(g16, ref), rel_rms(g8, g16)
    print(f"{name}: e_q {e_q:.3e}  gpu_int8/ref {r8:.3e} ({r8 / e_q:.3f} e_q)  "
          f"gpu_int8/gpu_fp16 {r816:.3e} ({r816 / e_q:.3f} e_q)  gpu_fp16/ref {r16:.2e}")
    assert 5e-3 < e_q < 0.1, e_q                # the fake quantisation did something sane
    assert r8 <= 1.25 * e_q, (r8, e_q)
    assert r816 >= 0.5 * e_q, (r816, e_q)       # the int8 path actually ran
    assert e8.encoder_compute == "int8"
    return g8, g16


def test_int8_encoder_tiny(tiny):
    encoder_against_oracle(*tiny, "tiny.en seed 5")


def test_int8_encoder_base(gpu):
    cfg = CONFIGS["base.en"]
    W = synthetic_weights(cfg, seed=7)
    e8 = WhisperEngine(cfg, W, encoder_compute="int8")
    e16 = WhisperEngine(cfg, W)
    pcm, offs = pack([synth_speech(31, 9.0)], gpu)
    mel = e16.logmel(pcm, offs, 1, 3)
    encoder_against_oracle(cfg, W, e8, e16, mel, "base.en seed 7")


# ------------------------------------------------------------------ 5. switching modes
def test_switching_modes(tiny, gpu):
    cfg, W, e8, e16, mel = tiny
    eng = WhisperEngine(cfg, W, encoder_compute="int8")
    first = eng.encode(mel).clone()
    assert torch.equal(first, e8.encode(mel))
    eng.set_encoder_compute("float16")
    assert eng.encoder_compute == "float16"
    assert torch.equal(eng.encode(mel), e16.encode(mel))      # a fresh default engine's bits
    eng.set_encoder_compute("int8")
    assert eng.encoder_compute == "int8"
    assert torch.equal(eng.encode(mel), first)
    assert not torch.equal(first, e16.encode(mel))
    with pytest.raises(ValueError):
        eng.set_encoder_compute("int4")
    with pytest.raises(ValueError):
        WhisperEngine(cfg, W, encoder_compute="bfloat16")
    assert eng.encoder_compute == "int8"


# -------------------------------------------------------- 6. set_tensor re-quantises
def test_set_tensor_requantises(tiny, gpu):
    cfg, W, e8, e16, mel = tiny
    eng = WhisperEngine(cfg, W, encoder_compute="int8")
    before = eng.encode(mel).clone()
    name = "encoder.layers.1.fc1.weight"
    w2 = (np.asarray(W[name], np.float32) * 1.5).astype(np.float16).astype(np.float32)
    w2[3] = -w2[3]
    eng.set_tensor(name, w2)
    after = eng.encode(mel)
    fresh = WhisperEngine(cfg, {**W, name: w2}, encoder_compute="int8")
    assert torch.equal(after, fresh.encode(mel))
    assert not torch.equal(after, before)


# ------------------------------------------------------------------------- 7. wiring
def test_pipeline_int8_wiring(gpu):
    from janus_amd.pipeline import JanusPipeline
    from janus_amd.services.transcriber import generate_segments
    pipe = JanusPipeline(model="tiny.en", whisper_compute="int8", temperatures=(0.0,), max_length=12)
    assert pipe.whisper.encoder_compute == "int8"
    utts = [synth_speech(610, 2.0), synth_speech(611, 3.5)]
    pcm, offs = pack(utts, gpu)
    res = pipe.encode(pcm, offs, [len(u) for u in utts], timestamp=11.0)
    eng = WhisperEngine(CONFIGS["tiny.en"], seed=0, encoder_compute="int8")
    streams = generate_segments(eng, [np.ascontiguousarray(u[::3]) for u in utts], max_length=12,
                                temperatures=(0.0,))
    for b, st in enumerate(streams):
        text = st.transcript()
        assert res.texts[b] == text
        tags = OracleProsody(48000).analyze_buffer(utts[b])[0]
        assert res.packets[b] == (opk.serialize(text, 0, tags, "auto", 11.0) if text.strip() else None)
    assert JanusPipeline(model="tiny.en", temperatures=(0.0,), max_length=12).whisper.encoder_compute == "float16"


def test_whisper_model_compute_type(gpu):
    from janus_amd.services.transcriber import WhisperModel
    m = WhisperModel("tiny.en", device="cpu", compute_type="int8")
    assert m.effective_compute_type == "float16" and m.engine.encoder_compute == "float16"
    assert m.requested_compute_type == "int8"
    m8 = WhisperModel("tiny.en", device="cpu", compute_type="int8", apply_compute_type=True)
    assert m8.effective_compute_type == "int8_float16" and m8.engine.encoder_compute == "int8"
    mf = WhisperModel("tiny.en", device="cpu", compute_type="float32", apply_compute_type=True)
    assert mf.effective_compute_type == "float16" and mf.engine.encoder_compute == "float16"
