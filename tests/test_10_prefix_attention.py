"""Prefix form of the Phi attention (image sessions: N prompts share their first P rows): psalm_causal_attention_f32_prefix[_split] and the
cache producer psalm_phi_prefix_kv_store against a plain torch restatement on the concatenated P + S sequence, and against the prefill
kernel.  Runs on the host emulation of the kernels here and on the real GPU under `-m gpu`."""
import pytest
import torch

from ops_backend import ops  # noqa: F401

HD, ROT = 64, 32


def tol(want):                                     # tests/test_1_ops.py tol(torch.float32, scale)
    return 3e-5 * want.abs().max()


def _rope_tables(L, rot=ROT, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    fr = torch.arange(L, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat((fr, fr), -1)
    return emb.cos().contiguous(), emb.sin().contiguous()


def _rope(x, cos, sin):
    xr = x[..., :ROT]
    rh = torch.cat((-xr[..., ROT // 2:], xr[..., : ROT // 2]), -1)
    return torch.cat((xr * cos + rh * sin, x[..., ROT:]), -1)


_DATA = {}


def _case(N, P, S, heads):
    """Inputs + the torch reference of one shape, computed once and shared (never modified) by the tests that need it.
    Buffers: column blocks q at 0, k at H + 8, v at 2H + 16 of rows of 3H + 16 floats (as test_causal_attention)."""
    key = (N, P, S, heads)
    if key in _DATA:
        return _DATA[key]
    H = heads * HD
    g = torch.Generator().manual_seed(100 * N + P + S + heads)
    ld = 3 * H + 16
    pre = torch.randn(P, ld, generator=g) * 0.8                   # the shared prefix rows
    suf = torch.randn(N * S, ld, generator=g) * 0.8               # the suffix rows of the N prompts
    mask = torch.ones(N, S, dtype=torch.uint8)
    if N > 1:
        mask[1, S - 7:] = 0                                       # the last 7 suffix keys of prompt 1 are padding
    cos, sin = _rope_tables(P + S)
    want = torch.zeros(N * S, H)
    L = P + S
    for n in range(N):
        full = torch.cat((pre, suf[n * S:(n + 1) * S]))
        q = full[:, 0:H].view(L, heads, HD).transpose(0, 1)
        k = full[:, H + 8:2 * H + 8].view(L, heads, HD).transpose(0, 1)
        v = full[:, 2 * H + 16:3 * H + 16].view(L, heads, HD).transpose(0, 1)
        km = torch.cat((torch.ones(P, dtype=torch.uint8), mask[n])).bool()
        w_ = _rope(q, cos, sin) @ _rope(k, cos, sin).transpose(1, 2) * HD ** -0.5
        allow = torch.tril(torch.ones(L, L, dtype=torch.bool))[None] & km[None, None, :]
        w_ = w_.masked_fill(~allow, torch.finfo(torch.float32).min).softmax(-1)
        want[n * S:(n + 1) * S] = (w_ @ v).transpose(0, 1).reshape(L, H)[P:]
    _DATA[key] = dict(pre=pre, suf=suf, mask=mask, cos=cos, sin=sin, want=want, H=H, ld=ld)
    return _DATA[key]


def _cache(ops, c, P, heads):
    """the prefix cache of one layer, written by psalm_phi_prefix_kv_store from the prefix rows' buffer"""
    d = ops.device
    Pp = (P + 31) // 32 * 32
    kc = torch.full((heads, Pp, HD), float("nan"), device=d)     # (the producer must write every row, padding included)
    vc = torch.zeros(P, c["H"], device=d)
    ops.phi_prefix_kv_store(c["pre"].to(d), c["H"] + 8, 2 * c["H"] + 16, c["cos"].to(d), c["sin"].to(d), kc, vc, P, heads, HD, ROT)
    return kc, vc


SHAPES = [(1, 40, 70, 2),        # P inside a tile, S over two tile edges
          (3, 64, 33, 1),        # P exactly two tiles, S one past a tile, shared prefix with N > 1
          (2, 1, 100, 4),        # one-key prefix
          (2, 130, 20, 8)]       # heads * N % 8 == 0: XCD placement active; last 7 suffix keys of prompt 1 masked


@pytest.mark.parametrize("N,P,S,heads", SHAPES)
def test_prefix_attention_vs_torch(ops, N, P, S, heads):
    c = _case(N, P, S, heads)
    d, H = ops.device, c["H"]
    kc, vc = _cache(ops, c, P, heads)
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.zeros(N * S, H + 32, device=d)
    ops.causal_attention_prefix(c["suf"].to(d), 0, H + 8, 2 * H + 16, kc, vc, out, 32, c["cos"].to(d), c["sin"].to(d), c["mask"].to(d),
                                N, S, P, heads, HD, ROT)
    got = out[:, 32:].cpu()
    err = (got - c["want"]).abs().max()
    print(f"prefix attention (N={N}, P={P}, S={S}, heads={heads}): max err {err:.3e}, bound {tol(c['want']):.3e}")
    assert torch.isfinite(got).all()
    assert err <= tol(c["want"])
    assert out[:, :32].abs().max() == 0                           # padding columns of the output buffer untouched
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)          # the prefix cache is read only
    assert (kc[:, P:] == 0).all()                                 # ... and its padding rows are zeros


@pytest.mark.parametrize("P,S,heads", [(40, 70, 2), (64, 33, 1), (1, 100, 4)])
def test_prefix_attention_vs_prefill_kernel(ops, P, S, heads):
    """N = 1: rows P .. P+S-1 of the prefill kernel on the concatenated buffer.  Not bitwise: the two kernels deal key tiles to waves differently."""
    c = _case(1, P, S, heads)
    d, H, L = ops.device, c["H"], P + S
    full = torch.cat((c["pre"], c["suf"])).to(d)
    ref = torch.zeros(L, H, device=d)
    ops.causal_attention(full, 0, H + 8, 2 * H + 16, ref, 0, c["cos"].to(d), c["sin"].to(d), torch.ones(1, L, dtype=torch.uint8, device=d), 1, L,
                         heads, HD, ROT)
    kc, vc = _cache(ops, c, P, heads)
    out = torch.zeros(S, H, device=d)
    ops.causal_attention_prefix(c["suf"].to(d), 0, H + 8, 2 * H + 16, kc, vc, out, 0, c["cos"].to(d), c["sin"].to(d), c["mask"].to(d), 1, S, P,
                                heads, HD, ROT)
    diff = (out.cpu() - ref[P:].cpu()).abs().max()
    print(f"prefix vs prefill kernel (P={P}, S={S}, heads={heads}): max difference {diff:.3e}")
    assert diff <= tol(c["want"])


@pytest.mark.parametrize("N,P,S,heads", [(1, 40, 70, 2), (2, 130, 20, 4)])
def test_prefix_attention_split_output(ops, N, P, S, heads):
    """the _split entry == the plain entry followed by a split under the given per-row scales (test_causal_attention_split_output's assertion)"""
    c = _case(N, P, S, heads)
    d, Hh = ops.device, c["H"]
    g = torch.Generator().manual_seed(17)
    kc, vc = _cache(ops, c, P, heads)
    args = (c["cos"].to(d), c["sin"].to(d), c["mask"].to(d), N, S, P, heads, HD, ROT)
    ref = torch.zeros(N * S, Hh, device=d)
    ops.causal_attention_prefix(c["suf"].to(d), 0, Hh + 8, 2 * Hh + 16, kc, vc, ref, 0, *args)
    ref = ref.cpu()
    vmax = torch.maximum(c["suf"][:, 2 * Hh + 16:].abs().max(), c["pre"][:, 2 * Hh + 16:].abs().max())
    inv = torch.exp2(torch.ceil(torch.log2(vmax)) - 12 + torch.randint(0, 4, (N * S,), generator=g).float())    # |v| / inv < 2^13
    off = 64
    Kp = (off + Hh + 63) // 64 * 64 + 64
    so = torch.zeros(N * S, 2 * Kp, dtype=torch.float16, device=d)
    ops.causal_attention_prefix_split(c["suf"].to(d), 0, Hh + 8, 2 * Hh + 16, kc, vc, so, inv.to(d), off, *args)
    so = so.cpu()
    hi, lo = so[:, off:off + Hh].double(), so[:, Kp + off:Kp + off + Hh].double()
    rec = (hi + lo) * inv.double()[:, None]
    assert ((rec - ref.double()).abs() <= 2.0 ** -21 * ref.abs().double() + 2.0 ** -24 * inv.double()[:, None]).all()
    assert hi.abs().max() < 2.0 ** 13
    mask = torch.ones(2 * Kp, dtype=torch.bool)
    mask[off:off + Hh] = False
    mask[Kp + off:Kp + off + Hh] = False
    assert (so[:, mask] == 0).all()


@pytest.mark.parametrize("P,heads", [(40, 2), (64, 1), (130, 4)])
def test_prefix_cache_producer_matches_the_prefill_pre_pass(ops, P, heads):
    """The K cache == what phi_rope_prep_f32_kernel leaves in the prefill kernel's workspace for those rows (same arithmetic on the same values:
    bitwise), V == the buffer's v columns.  This is the producer kernel alone, on one buffer; the prefix PASS's cache (its own GEMM, M = P rows) against
    the one-shot pass's K / V for the same rows (M = B * L) is tests/test_11_session_emu.py::test_prefix_pass_cache_is_the_one_shot_pass_rows and,
    on the GPU, tests/test_12_session_gpu.py::test_prefix_pass_cache_vs_one_shot_pass_rows_on_gpu."""
    c = _case(*{(40, 2): (1, 40, 70, 2), (64, 1): (3, 64, 33, 1), (130, 4): (2, 130, 20, 4)}[(P, heads)])
    d, H = ops.device, c["H"]
    Pp = (P + 31) // 32 * 32
    kc, vc = _cache(ops, c, P, heads)
    out = torch.zeros(P, H, device=d)
    ops.causal_attention(c["pre"].to(d), 0, H + 8, 2 * H + 16, out, 0, c["cos"].to(d), c["sin"].to(d), torch.ones(1, P, dtype=torch.uint8, device=d),
                         1, P, heads, HD, ROT)
    ops.lib.psalm_causal_attention_f32_workspace.restype = __import__("ctypes").c_long
    nbytes = ops.lib.psalm_causal_attention_f32_workspace(1, P, heads)
    ws = ops._ws[("causal_f32_ws", nbytes)]                       # [Qr | Kr | mask bytes]: Kr is the second (heads, Pp, 64) block
    n = heads * Pp * HD
    kr = ws[4 * n:8 * n].view(torch.float32).view(heads, Pp, HD)
    assert torch.equal(kc.cpu(), kr.cpu())
    assert torch.equal(vc.cpu(), c["pre"][:, 2 * H + 16:3 * H + 16])
