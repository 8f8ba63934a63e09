"""Attention kernels at trained-model logit ranges.

Every other attention test draws q, k, v from randn * 0.7 .. 1.0: the logits of a row then span a unit or two, the running maximum of an online
softmax barely moves and every rescale factor is close to 1.  Here ONE input builder gives each (batch / window, head) a unit direction u and sets
q_i = a u + noise, k_j = c_j u + noise with a = 1 / scale, so the logit of (i, j) is c_j (+ noise of a fraction of a unit) and the PROFILE c_j is the
test's to choose.  u lives in the head dims RoPE leaves alone (the noise is rotated), the q noise is orthogonal to u, and the float64 reference
applies the same RoPE, bias and masks on the inputs exactly as the kernel receives them (after the bf16 rounding for bf16 cases).

Profiles
  rising        c_j climbs STEP per key tile of the kernel under test: the running maximum rises by >= 20 in every tile.  Tiles: 32 keys (fp32 causal /
                prefix / grouped: four wavefronts are dealt the tiles round-robin, so each private state jumps by 4 STEP and the LDS merge sees maxima
                STEP .. 3 STEP apart), 64 (bf16 causal), the chunk of psalm_mha_attention_f32 (64 .. 256 keys: 64 at these shapes, one partial state
                per chunk for the combine kernel), the split of psalm_mha_attention_mfma (64 at these shapes), 16 (the matrix-core window kernels'
                key tiles), 4 (the rescale group of the scalar kernels).
  falling       the reverse: the maximum is fixed after the first tile, later tiles add probabilities down to underflow.
  spike         a flat row with one key SPIKE = 100 above the rest: last key of the ragged last tile (= the last chunk only, for split-KV MHA: the
                other chunks merge with exp(m_w - M) = 0), first key, the key before the right padding, a diagonal key, the last prefix key
                (P % 32 != 0), the first suffix key -- dealt over the (batch, head) pairs of a case.
  masked_spike  the largest logit of a row, >= 80 above every visible one, sits on a key that does not count: a causal-future key, a
                key_mask == 0 key, an MHA mask == 1 key.  The flagged all-masked MHA row attends everywhere, the spike included.
  shift         shifted windows: every key's logit is >= 40 higher for the queries across the shift-mask boundary than for those of its own region
                (most keys 70, every third 100; bias table and noise take up to ~25 of that), on top of a falling ramp of span 70.  The additive -100 leaves the 70-keys at exp(-30) and the
                100-keys at full weight: a hard mask, or a flavour that forgot the mask, moves the output by far more than the bar (asserted on
                the reference).  Reference mask: oracle swin_shift_mask.
In every profile v carries a few entries of 1e3 on keys whose reference probability is < 1e-20 for every query: a leak through a wrong rescale
shows at full size.

Asserted on the REFERENCE before the kernel is looked at: raw (un-masked) logit span of every row >= 60; rising: per-tile maxima of the visible
logits climb by >= 20 at every tile boundary; masked_spike: the masked logit exceeds every visible one by >= 80 on some rows of every
(batch, head); every output row finite and non-zero.

Bars.  bf16 kernels: 2^-7 max|want| (probabilities lie in [0, 1]: independent of the logit range).  _split forms: hi + lo == the plain fp32
kernel's output to 22 bits, |hi| < 2^13, nothing outside the addressed columns written.  fp32 kernels: max(3e-5 max|want|, 4 e32) with e32 the
worst error of the same formula evaluated in torch float32 against float64 -- the rounding error of the logits themselves grows with their
magnitude, so no fixed number carries over; the 4 covers another summation order and the hardware exp, it is a margin over a plain fp32
evaluation, never derived from the kernel's output.

Measured err_kernel / max(e32, 7.5e-6 max|want|), worst case per family over every profile and shape, from this file run with -s (the
[range] lines).  "emu" is the host emulation of the kernels (libm exp); "MI355X" is one run of this file under `-m gpu` on an MI355X (gfx950)
with the library built by psalm_amd.build (146 cases, 4 s).  The two columns agree because at these ranges the error is the fp32 rounding of
the logits, not the exp: no family comes near the factor 4.
  family                              emu     MI355X
  window_f32_mfma (K through LDS)     1.44    1.44
  window_f32_mfma (one wavefront)     1.14    1.14
  window_f32_split (its plain run)    1.02    1.03
  window_scalar                       1.47    1.47
  causal_f32_splitk                   1.31    1.31
  causal_f32_split (its plain run)    0.49    0.49
  causal_scalar                       1.04    1.00
  prefix_f32                          1.67    1.67
  prefix_f32_split (its plain run)    1.44    1.44
  grouped_f32 / grouped_f32_split     1.62    1.62
  mha_f32_mfma + combine              0.96    0.96
  mha_scalar_f32                      1.03    1.03
bf16 families, worst err as a fraction of the 2^-7 max|want| bar (the same on both): window 0.46, causal 0.43, split-KV MHA 0.42, scalar MHA 0.30.
"""
import math

import pytest
import torch

from ops_backend import ops  # noqa: F401
from oracle import psalm_oracle as O

STEP, STEP_WIN, SPIKE, NOISE = 26.0, 30.0, 100.0, 0.25
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the one input builder
def unit_dirs(g, lead, hd, lo=0, ortho=1):
    """(*lead, ortho, hd): `ortho` orthonormal directions per leading index, supported on head dims lo.. (RoPE leaves dims >= rot alone)"""
    m = torch.randn(*lead, hd - lo, ortho, generator=g, dtype=F64)
    qm = torch.linalg.qr(m).Q.transpose(-1, -2)
    out = torch.zeros(*lead, ortho, hd, dtype=F64)
    out[..., lo:] = qm
    return out


def directed(g, u, amp, orth=False):
    """amp (*lead, L) along u (*lead, hd) + noise -> (*lead, L, hd); orth: noise orthogonal to u (a query's noise then does not scale the profile)"""
    n = torch.randn(*amp.shape, u.shape[-1], generator=g, dtype=F64) * NOISE
    uu = u.unsqueeze(-2)
    if orth:
        n = n - (n * uu).sum(-1, keepdim=True) * uu
    return amp.unsqueeze(-1) * uu + n


def ramp(tile_id, step):
    """c_j = step * tile + a small climb inside the tile, centred on 0"""
    t = tile_id.to(F64)
    inside = torch.zeros_like(t)
    for v in t.unique():
        sel = t == v
        inside[sel] = torch.arange(int(sel.sum()), dtype=F64) / max(1, int(sel.sum()))
    c = step * t + 0.1 * step * inside
    return c - (c.max() + c.min()) / 2


def plant_large_v(g, v, pmax):
    """v (*lead, Lk, hd), pmax (*lead, Lk) = each key's largest reference probability over the queries that share this v: up to 3 keys per leading
    index with pmax < 1e-20 get one entry of +-1e3.  Returns the number planted."""
    n = 0
    flat_v, flat_p = v.reshape(-1, *v.shape[-2:]), pmax.reshape(-1, pmax.shape[-1])
    for i in range(flat_v.shape[0]):
        cand = (flat_p[i] < 1e-20).nonzero().flatten()
        if cand.numel() == 0:
            continue
        pick = cand[torch.randperm(cand.numel(), generator=g)[:3]]
        for j in pick.tolist():
            d = int(torch.randint(0, v.shape[-1], (1,), generator=g))
            flat_v[i, j, d] = 1e3 if (j + d) % 2 else -1e3
            n += 1
    return n


def attend(q, k, v, scale, add=None, allow=None):
    """softmax((q scale) k^T + add, masked where ~allow) v in the dtype of the operands -> (raw logits before the mask, probabilities, output)"""
    raw = (q * scale) @ k.transpose(-1, -2)
    if add is not None:
        raw = raw + add
    s = raw if allow is None else raw.masked_fill(~allow, float("-inf"))
    p = s.softmax(-1)
    return raw, p, p @ v


# ------------------------------------------------------------------------------------------------ the conditions on the reference
def check_reference(raw, allow, want, profile, tile_id=None):
    """raw (..., Lq, Lk) float64 un-masked logits, allow (..., Lq, Lk) bool or None, want (..., Lq, hd), tile_id (Lk) or (..., 1, Lk)"""
    span = raw.amax(-1) - raw.amin(-1)
    assert span.min() >= 60, f"profile degenerate: smallest row span {span.min():.1f}"
    assert torch.isfinite(want).all() and (want.abs().amax(-1) > 0).all()
    vis = raw if allow is None else raw.masked_fill(~allow, float("-inf"))
    if profile == "rising":
        tid = tile_id.expand(*raw.shape[:-2], 1, raw.shape[-1]) if tile_id.dim() > 1 else tile_id.view(*([1] * (raw.dim() - 1)), -1)
        nt = int(tile_id.max()) + 1
        tmax = torch.stack([vis.masked_fill(tid != t, float("-inf")).amax(-1) for t in range(nt)], -1)          # (..., Lq, tiles)
        both = torch.isfinite(tmax[..., 1:]) & torch.isfinite(tmax[..., :-1])
        rise = (tmax[..., 1:] - tmax[..., :-1])[both]
        assert rise.numel() > 0 and rise.min() >= 20, f"rising: smallest tile-to-tile rise {rise.min():.1f}"
    if profile == "masked_spike":
        hidden = raw.masked_fill(allow, float("-inf")).amax(-1)
        margin = hidden - vis.amax(-1)
        hit = margin > 40                                                         # the rows whose largest logit is the masked spike
        assert hit.any(-1).all(), "masked_spike: a (batch, head) without a masked spike"
        assert margin[hit].min() >= 80, f"masked_spike: margin {margin[hit].min():.1f}"


def report(name, profile, got, want, e32):
    """the figure before the assertion: [range] lines feed the table of the module docstring"""
    err = float((got.double() - want).abs().max())
    wmax = float(want.abs().max())
    if e32 is None:
        print(f"[range] {name} {profile}: err {err:.3e}  bar(2^-7) {2 ** -7 * wmax:.3e}")
        return err, 2 ** -7 * wmax
    bar = max(3e-5 * wmax, 4 * e32)
    print(f"[range] {name} {profile}: err {err:.3e}  e32 {e32:.3e}  err/e32 {err / max(e32, 7.5e-6 * wmax):.2f}  bar {bar:.3e}")
    return err, bar


def check_split(so, inv, ref, off, Hh, Kp):
    """the contract of every _split form (tests/test_1_ops.py::test_causal_attention_split_output)"""
    so = so.cpu()
    hi, lo = so[:, off:off + Hh].double(), so[:, Kp + off:Kp + off + Hh].double()
    rec = (hi + lo) * inv.double()[:, None]
    assert ((rec - ref.double()).abs() <= 2.0 ** -21 * ref.abs().double() + 2.0 ** -24 * inv.double()[:, None]).all()
    assert hi.abs().max() < 2.0 ** 13
    mask = torch.ones(2 * Kp, dtype=torch.bool)
    mask[off:off + Hh] = False
    mask[Kp + off:Kp + off + Hh] = False
    assert (so[:, mask] == 0).all()


_CASES = {}


def cached(fn):
    def wrap(*key):
        if (fn.__name__, key) not in _CASES:
            _CASES[(fn.__name__, key)] = fn(*key)
        return _CASES[(fn.__name__, key)]
    return wrap


# ================================================================================================ Swin window attention
WS, HDW = 12, 32
WINDOW = [("f32", 1, 2, 3, 2, 6), ("f32", 2, 2, 2, 2, 0), ("bf16", 1, 2, 3, 2, 6), ("bf16", 2, 2, 2, 2, 0),
          ("f32", 1, 6, 7, 16, 6),            # 672 (window, head) pairs: the one-wavefront flavour of the fp32 matrix-core kernel
          ("split", 1, 2, 2, 4, 6),           # psalm_window_attention_split
          ("scalar", 1, 2, 3, 2, 6)]          # a 4-byte aligned fp32 buffer: the per-thread window_attention_kernel


@cached
def window_case(kind, B, nWh, nWw, heads, shift, profile):
    from psalm_amd.synthetic import relative_position_index
    N, nW, scale = WS * WS, nWh * nWw, HDW ** -0.5
    nb = B * nW
    g = torch.Generator().manual_seed(1000 + 7 * heads + nb + len(profile))
    dirs = unit_dirs(g, (nb, heads), HDW, ortho=5)                   # u and four region directions
    u = dirs[..., 0, :]
    tile = 4 if kind == "scalar" else 16
    j = torch.arange(N)
    if profile in ("rising", "falling"):
        c = ramp(j // tile, STEP_WIN) * (1 if profile == "rising" else -1)
        c = c.expand(nb, heads, N)
    elif profile == "spike":
        c = torch.zeros(nb, heads, N, dtype=F64)
        for b in range(nb):
            for h in range(heads):
                c[b, h, [N - 1, 0, 77, 16][(b + h) % 4]] = SPIKE     # last key (tile 8 of 9 / the padded fifth 32-tile of the bf16 kernel), first, ...
    else:                                                            # shift
        c = (-ramp(j // 1, 70.0 / N)).expand(nb, heads, N)
    q = directed(g, u, torch.full((nb, heads, N), 1 / scale, dtype=F64), orth=True)
    k = directed(g, u, c.contiguous())
    am = O.swin_shift_mask(nWh * WS, nWw * WS, WS, shift).double() if shift else None        # (nW, N, N): 0 / -100
    if profile == "shift":
        gain = torch.where(j % 3 == 0, 100.0, 70.0).double()
        for w in range(nW):
            same = am[w] == 0
            rep = same.float().argmax(1)                             # a token's region: its first same-region token
            regs = rep.unique().tolist()
            assert len(regs) <= 4
            for b in range(B):
                for r, t0 in enumerate(regs):
                    e = dirs[b * nW + w, :, 1 + r, :]                # (heads, hd)
                    kw, qw = k[b * nW + w], q[b * nW + w]            # (heads, N, hd) views
                    kw[:, rep == t0] += gain[rep == t0][None, :, None] * e[:, None, :]
                    if len(regs) > 1:
                        qw[:, rep != t0] += (1 / scale) * e[:, None, :]
    v = torch.randn(nb, heads, N, HDW, generator=g, dtype=F64)
    table = torch.randn((2 * WS - 1) ** 2, heads, generator=g)
    dt = torch.bfloat16 if kind == "bf16" else torch.float32
    q, k = q.float().to(dt), k.float().to(dt)
    bias = table[relative_position_index(WS).view(-1)].view(N, N, heads).permute(2, 0, 1)[None]
    add = bias if am is None else bias[:, None] + am[None, :, None]                          # (1, B?, nW, heads, N, N)
    if am is not None:
        add = add.expand(B, nW, heads, N, N).reshape(nb, heads, N, N)
    raw, p, _ = attend(q.double(), k.double(), v, scale, add.double())
    plant_large_v(g, v, p.amax(-2))
    v = v.float().to(dt)
    raw, p, want = attend(q.double(), k.double(), v.double(), scale, add.double())
    raw_nomask = raw - (0 if am is None else am[None, :, None].expand(B, nW, heads, N, N).reshape(nb, heads, N, N))
    check_reference(raw_nomask, None, want, profile, j // tile)
    e32 = None
    if kind != "bf16":
        e32 = float((attend(q.float(), k.float(), v.float(), scale, add.float())[2].double() - want).abs().max())
    if profile == "shift":
        cross = (am != 0)[None, :, None].expand(B, nW, heads, N, N).reshape(nb, heads, N, N)
        lo_ = raw_nomask.masked_fill(~cross, float("inf")).amin(-2)                          # a key seen from across the boundary ...
        hi_ = raw_nomask.masked_fill(cross, float("-inf")).amax(-2)                          # ... and from its own region
        has = cross.any(-2)
        assert has.any() and (lo_ - hi_)[has].min() >= 40
        hard = attend(q.double(), k.double(), v.double(), scale, add.double().masked_fill(cross, float("-inf")))[2]
        nomask = attend(q.double(), k.double(), v.double(), scale, bias.double())[2]
        bar = 2 ** -7 * want.abs().max()
        assert (hard - want).abs().max() > 20 * bar and (nomask - want).abs().max() > 20 * bar
    qkv = torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(nb * N, 3 * heads * HDW).contiguous()
    return dict(qkv=qkv, table=table, want=want.transpose(1, 2).reshape(nb * N, heads * HDW), e32=e32)


@pytest.mark.parametrize("kind,B,nWh,nWw,heads,shift,profile",
                         [(*w, p) for w in WINDOW for p in ("rising", "falling", "spike", "shift") if p != "shift" or w[-1]])   # (shift: shifted cases)
def test_window_attention_range(ops, kind, B, nWh, nWw, heads, shift, profile):
    c = window_case(kind, B, nWh, nWw, heads, shift, profile)
    d, qkv, want = ops.device, c["qkv"], c["want"]
    C = heads * HDW
    if kind == "scalar":
        flat = torch.zeros(qkv.numel() + 1)
        flat[1:] = qkv.reshape(-1)
        qd = flat.to(d)[1:].view(qkv.shape)
        assert qd.data_ptr() % 16 != 0
    else:
        qd = qkv.to(d)
    if kind == "split":
        rows = qkv.shape[0]
        g = torch.Generator().manual_seed(5)
        a_inv = torch.exp2(torch.randint(-14, -8, (rows,), generator=g).float())
        par = torch.tensor([float((qkv[:, 2 * C:].abs().amax(1) / a_inv).max()) * 1.01, 0.25])
        ref = ops.window_attention(qd, c["table"].to(d), B, nWh, nWw, heads, WS, shift).cpu()
        got = ops.window_attention_split(qd, c["table"].to(d), a_inv.to(d), par.to(d), B, nWh, nWw, heads, WS, shift)
        t, inv = got.t.cpu(), got.inv_scale.cpu().double()
        hi, lo = t[:, :C].double(), t[:, got.Kp:got.Kp + C].double()
        assert ((hi + lo) * inv[:, None] - ref.double()).abs().max() <= 2.0 ** -21 * ref.abs().max() and hi.abs().max() < 2.0 ** 13
        if got.Kp > C:
            assert (t[:, C:got.Kp] == 0).all() and (t[:, got.Kp + C:] == 0).all()
        err, bar = report("window_f32_split_plain_kernel", profile, ref, want, c["e32"])
        assert err <= bar
        return
    # (host emulation only: probabilities that underflow are denormal arithmetic at a tenth of the speed on a CPU -- 34 s against 11 s for the 672-pair
    # case; flushed for the duration of the call, which moves nothing above 1e-38)
    ftz = ops.is_emu and torch.set_flush_denormal(True)
    try:
        got = ops.window_attention(qd, c["table"].to(d), B, nWh, nWw, heads, WS, shift).cpu()
    finally:
        if ftz:
            torch.set_flush_denormal(False)
    name = {"f32": "window_f32_mfma_1wave" if B * nWh * nWw * heads > 640 else "window_f32_mfma_klds", "bf16": "window_bf16_mfma",
            "scalar": "window_scalar"}[kind]
    err, bar = report(name, profile, got, want, c["e32"])
    assert torch.isfinite(got.float()).all() and err <= bar


# ================================================================================================ Phi causal / prefix / grouped prefix attention
HD, ROT = 64, 32


def rope_tables(L, rot=ROT, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    fr = torch.arange(L, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat((fr, fr), -1)
    return emb.cos().contiguous(), emb.sin().contiguous()


def rope(x, cos, sin):
    xr = x[..., :ROT]
    rh = torch.cat((-xr[..., ROT // 2:], xr[..., : ROT // 2]), -1)
    return torch.cat((xr * cos + rh * sin, x[..., ROT:]), -1)


# kind, heads, per-prompt prefix lengths, per-prompt group, S, per-prompt right padding
SEQ = {
    "causal_f32_300": ("f32", 2, [0, 0], None, 300, [0, 20]),
    "causal_f32_129": ("f32", 1, [0], None, 129, [0]),
    "causal_bf16_300": ("bf16", 2, [0, 0], None, 300, [0, 20]),
    "causal_bf16_129": ("bf16", 1, [0], None, 129, [0]),
    "causal_split_70": ("split", 4, [0, 0], None, 70, [0, 20]),
    "causal_scalar_129": ("scalar", 1, [0], None, 129, [0]),                       # k_off % 4 != 0: the per-thread causal_attention_kernel
    "prefix_40_70": ("prefix", 2, [40], [0], 70, [0]),                             # tests/test_10 SHAPES[0]: P % 32 != 0
    "prefix_64_33": ("prefix", 1, [64, 64, 64], [0, 0, 0], 33, [0, 7, 0]),         # SHAPES[1]
    "prefix_split_130_20": ("prefix_split", 4, [130, 130], [0, 0], 20, [0, 7]),
    "grouped_three_caches": ("grouped", 2, [40, 64, 1], [0, 1, 2], 70, [0, 7, 0]),     # tests/test_16 A (P % 32 != 0)
    "grouped_shared_cache": ("grouped", 4, [130, 130, 33, 97], [0, 0, 1, 2], 20, [0, 7, 0, 0]),   # B
    "grouped_split": ("grouped_split", 4, [130, 130, 33, 97], [0, 0, 1, 2], 20, [0, 7, 0, 0]),
}


@cached
def seq_case(name, profile):
    kind, heads, Ps, groups, S, pads = SEQ[name]
    N, H, scale = len(Ps), heads * HD, HD ** -0.5
    tile = {"bf16": 64, "scalar": 4}.get(kind, 32)
    g = torch.Generator().manual_seed(2000 + sum(Ps) + S + heads + len(profile))
    u = unit_dirs(g, (heads,), HD, lo=ROT)[:, 0]                     # (heads, hd), zero in the rotated dims
    G = (max(groups) + 1) if groups else 0
    gP = [0] * G
    for n in range(N):
        if groups:
            gP[groups[n]] = Ps[n]
    ptiles = [(P + tile - 1) // tile for P in Ps]                    # the kernel's tile list: the prefix tiles, then the suffix tiles from suffix key 0

    def tile_id(n):
        jj = torch.arange(Ps[n] + S)
        return torch.where(jj < Ps[n], jj // tile, ptiles[n] + (jj - Ps[n]) // tile)
    tmax_all = max(int(tile_id(m).max()) for m in range(N))
    step = max(STEP, 70.0 / min(int(tile_id(m).max()) for m in range(N)))      # (a prompt of three tiles still spans 60)
    c_pre = [torch.zeros(heads, gP[i], dtype=F64) for i in range(G)]
    c_suf = [torch.zeros(heads, S, dtype=F64) for _ in range(N)]
    for n in range(N):
        P, L, real = Ps[n], Ps[n] + S, Ps[n] + S - pads[n]
        for h in range(heads):
            if profile in ("rising", "falling"):
                full = ramp(tile_id(n), step)
                full = (full - full[0] - 0.5 * step * tmax_all) * (1 if profile == "rising" else -1)   # a prefix position: one value whatever the prompt
            else:
                full = torch.zeros(L, dtype=F64)
                if profile == "spike":
                    cand = [real - 1, 0, P - 1 if P else S // 2 + 1, P if P else 32]       # ragged last tile / before the padding, first key,
                    pos = cand[(h + 3 * n) % 4]                                            # last prefix key or a diagonal, first suffix key
                    if pos < P and n != [m for m in range(N) if groups[m] == groups[n]][0]:
                        pos = P                                                            # (a prefix spike belongs to the group's first prompt)
                else:
                    pos = L - max(1, pads[n] // 2) if (pads[n] and h % 2 == 0) else P + S // 2 + 1   # a key_mask == 0 key / a causal-future key
                full[pos] = SPIKE
            if P and profile in ("rising", "falling"):
                c_pre[groups[n]][h] = full[:P]
            elif P:
                c_pre[groups[n]][h] = torch.maximum(c_pre[groups[n]][h], full[:P])
            c_suf[n][h] = full[P:]
    k_pre = [directed(g, u, c_pre[i]) for i in range(G)]             # (heads, P, hd)
    k_suf = [directed(g, u, c_suf[n]) for n in range(N)]
    q_pre = [directed(g, u, torch.full((heads, gP[i]), 1 / scale, dtype=F64), orth=True) for i in range(G)]      # (unused by the prefix kernels)
    q_suf = [directed(g, u, torch.full((heads, S), 1 / scale, dtype=F64), orth=True) for n in range(N)]
    v_pre = [torch.randn(heads, gP[i], HD, generator=g, dtype=F64) for i in range(G)]
    v_suf = [torch.randn(heads, S, HD, generator=g, dtype=F64) for n in range(N)]
    dt = torch.bfloat16 if kind == "bf16" else torch.float32
    rnd = lambda t: t.float().to(dt)                                 # noqa: E731
    k_pre, k_suf, q_suf, q_pre = [rnd(t) for t in k_pre], [rnd(t) for t in k_suf], [rnd(t) for t in q_suf], [rnd(t) for t in q_pre]
    Lmax = max(Ps) + S
    cos, sin = rope_tables(Lmax)

    def evaluate(f, vp, vs):
        outs = []
        for n in range(N):
            P, L = Ps[n], Ps[n] + S
            kf = torch.cat(([k_pre[groups[n]]] if P else []) + [k_suf[n]], 1).to(f)
            vf = torch.cat(([vp[groups[n]]] if P else []) + [vs[n]], 1).to(f)
            qr = rope(q_suf[n].to(f), cos[P:L].to(f), sin[P:L].to(f))
            kr = rope(kf, cos[:L].to(f), sin[:L].to(f))
            km = torch.ones(L, dtype=torch.bool)
            km[L - pads[n]:] = pads[n] == 0
            allow = (torch.arange(L)[None, :] <= (P + torch.arange(S))[:, None]) & km[None, :]
            outs.append(attend(qr, kr, vf, scale, None, allow[None].expand(heads, S, L)) + (allow,))
        return outs
    first = evaluate(F64, v_pre, v_suf)
    for i in range(G):
        pm = torch.stack([first[n][1][:, :, :gP[i]].amax(-2) for n in range(N) if groups[n] == i]).amax(0)
        plant_large_v(g, v_pre[i], pm)
    for n in range(N):
        plant_large_v(g, v_suf[n], first[n][1][:, :, Ps[n]:].amax(-2))
    v_pre, v_suf = [rnd(t) for t in v_pre], [rnd(t) for t in v_suf]
    ref = evaluate(F64, v_pre, v_suf)
    for n in range(N):
        raw, p, want, allow = ref[n]
        check_reference(raw, allow[None].expand_as(raw), want, profile, tile_id(n))
    want = torch.cat([r[2].transpose(0, 1).reshape(S, H) for r in ref])                    # (N * S, H)
    e32 = None
    if kind != "bf16":
        e32 = float((torch.cat([r[2].transpose(0, 1).reshape(S, H) for r in evaluate(torch.float32, v_pre, v_suf)]).double() - want).abs().max())
    k_off = H + 6 if kind == "scalar" else H + 8
    ld = 3 * H + 16

    def rows(q, k, v):                                               # (heads, R, hd) x 3 -> (R, ld) buffer rows
        R = q.shape[1]
        b = torch.zeros(R, ld, dtype=dt)
        b[:, 0:H] = q.transpose(0, 1).reshape(R, H)
        b[:, k_off:k_off + H] = k.transpose(0, 1).reshape(R, H)
        b[:, 2 * H + 16:] = v.transpose(0, 1).reshape(R, H)
        return b
    suf = torch.cat([rows(q_suf[n], k_suf[n], v_suf[n]) for n in range(N)])
    pre = [rows(q_pre[i], k_pre[i], v_pre[i]) for i in range(G)]
    mask = torch.ones(N, S, dtype=torch.uint8)
    for n in range(N):
        if pads[n]:
            mask[n, S - pads[n]:] = 0
    vmax = max([float(t.abs().max()) for t in v_pre + v_suf])
    return dict(kind=kind, heads=heads, Ps=Ps, groups=groups, gP=gP, S=S, N=N, H=H, ld=ld, k_off=k_off, suf=suf, pre=pre, mask=mask, cos=cos, sin=sin,
                want=want, e32=e32, vmax=vmax)


def _caches(ops, c):
    d, out = ops.device, []
    for pre, P in zip(c["pre"], c["gP"]):
        kc = torch.full((c["heads"], (P + 31) // 32 * 32, HD), float("nan"), device=d)
        vc = torch.zeros(P, c["H"], device=d)
        ops.phi_prefix_kv_store(pre.to(d), c["k_off"], 2 * c["H"] + 16, c["cos"].to(d), c["sin"].to(d), kc, vc, P, c["heads"], HD, ROT)
        out.append((None, [(kc, vc)]))
    return out


@pytest.mark.parametrize("profile", ["rising", "falling", "spike", "masked_spike"])
@pytest.mark.parametrize("name", list(SEQ))
def test_causal_and_prefix_attention_range(ops, name, profile):
    c = seq_case(name, profile)
    d, kind, H, N, S, heads = ops.device, c["kind"], c["H"], c["N"], c["S"], c["heads"]
    suf, cos, sin, mask = c["suf"].to(d), c["cos"].to(d), c["sin"].to(d), c["mask"].to(d)
    offs = (0, c["k_off"], 2 * H + 16)
    split = kind.endswith("split")
    if split:
        g = torch.Generator().manual_seed(17)
        inv = torch.exp2(math.ceil(math.log2(c["vmax"])) - 12 + torch.randint(0, 4, (N * S,), generator=g).float())      # |v| / inv < 2^13
        off = 64
        Kp = (off + H + 63) // 64 * 64 + 64
        so = torch.zeros(N * S, 2 * Kp, dtype=torch.float16, device=d)
    out = torch.zeros(N * S, H + 32, dtype=suf.dtype, device=d)
    if kind in ("f32", "bf16", "scalar", "split"):
        ops.causal_attention(suf, *offs, out, 32, cos, sin, mask, N, S, heads, HD, ROT)
        if split:
            ops.causal_attention_split(suf, *offs, so, inv.to(d), off, cos, sin, mask, N, S, heads, HD, ROT)
    elif kind.startswith("prefix"):
        kc, vc = _caches(ops, c)[0][1][0]
        ops.causal_attention_prefix(suf, *offs, kc, vc, out, 32, cos, sin, mask, N, S, c["Ps"][0], heads, HD, ROT)
        if split:
            ops.causal_attention_prefix_split(suf, *offs, kc, vc, so, inv.to(d), off, cos, sin, mask, N, S, c["Ps"][0], heads, HD, ROT)
    else:
        caches = _caches(ops, c)
        table = ops.prefix_ref_table(caches, c["groups"])[0]
        ops.causal_attention_prefix_grouped(suf, *offs, table, out, 32, cos, sin, mask, N, S, max(c["Ps"]), heads, HD, ROT)
        if split:
            ops.causal_attention_prefix_grouped_split(suf, *offs, table, so, inv.to(d), off, cos, sin, mask, N, S, max(c["Ps"]), heads, HD, ROT)
    got = out[:, 32:].cpu()
    assert out[:, :32].abs().max() == 0 and torch.isfinite(got.float()).all()
    if split:
        check_split(so, inv, got, off, H, Kp)
    family = {"f32": "causal_f32_splitk", "bf16": "causal_bf16_mfma", "scalar": "causal_scalar", "split": "causal_f32_split_plain_kernel",
              "prefix": "prefix_f32", "prefix_split": "prefix_f32_split_plain_kernel", "grouped": "grouped_f32",
              "grouped_split": "grouped_f32_split_plain_kernel"}[kind]
    err, bar = report(family, f"{name}/{profile}", got, c["want"], c["e32"])
    assert err <= bar


# ================================================================================================ predictor MHA
HDM = 32
# kind, B, heads, Lq, Lk
MHA = [("f32", 2, 4, 100, 1024), ("f32", 2, 4, 37, 203), ("f32", 2, 4, 12, 64), ("bf16t", 1, 8, 100, 1024), ("bf16t", 1, 8, 37, 200),
       ("scalar_f32", 2, 2, 10, 36), ("scalar_bf16", 2, 2, 10, 36)]


def mha_f32_chunk(B, heads, Lk):                                     # psalm_amd/csrc/attention.hip: mha_f32_chunk
    c = (Lk * heads * B + 1023) // 1024
    c = (c + 63) // 64 * 64
    return min(256, max(64, c))


def mha_mfma_split(B, heads, Lk):                                    # psalm_amd/csrc/attention_mfma.hip: mha_splits + psalm_mha_attention_mfma
    s = max(1, min((256 + heads * B - 1) // (heads * B), (Lk + 63) // 64))
    return ((Lk + s - 1) // s + 63) // 64 * 64


@cached
def mha_case(kind, B, heads, Lq, Lk, profile):
    scale = HDM ** -0.5
    tile = {"f32": mha_f32_chunk(B, heads, Lk), "bf16t": mha_mfma_split(B, heads, Lk)}.get(kind, 4)
    g = torch.Generator().manual_seed(3000 + Lq + Lk + len(profile))
    u = unit_dirs(g, (B, heads), HDM)[..., 0, :]
    j = torch.arange(Lk)
    mask = torch.rand(B, Lq, Lk, generator=g) < 0.3                  # 1 = blocked
    if profile in ("rising", "falling"):
        c = (ramp(j // tile, STEP) * (1 if profile == "rising" else -1)).expand(B, heads, Lk)
        if Lk <= tile:                                               # a single tile: the ramp inside it carries the span
            c = (ramp(j // 1, 70.0 / Lk) * (1 if profile == "rising" else -1)).expand(B, heads, Lk)
    else:
        c = torch.zeros(B, heads, Lk, dtype=F64)
        pos = torch.zeros(B, heads, dtype=torch.long)
        for b in range(B):
            for h in range(heads):
                pos[b, h] = [Lk - 1, 0, Lk // 2 + 1, Lk - 2][(b + h) % 4]      # the last key: ragged last tile, last chunk / split only
                c[b, h, pos[b, h]] = SPIKE
        if profile == "spike":
            mask[:, :, pos.flatten()] = False                        # the spikes are visible
        else:
            mask[:, :, pos.flatten()] = True                         # ... or blocked, for every query
    mask[0, 1, :] = True                                             # an all-masked row: flagged -> attends everywhere, a blocked spike included
    mask[B - 1, 2, : Lk - 3] = True                                  # a row whose only visible keys sit in the last chunk
    mask[B - 1, 2, Lk - 3:] = False
    flags = mask.all(-1)
    q = directed(g, u, torch.full((B, heads, Lq), 1 / scale, dtype=F64), orth=True)
    k = directed(g, u, c.contiguous())
    v = torch.randn(B, heads, Lk, HDM, generator=g, dtype=F64)
    dt = torch.float32 if kind.endswith("f32") else torch.bfloat16
    q, k = q.float().to(dt), k.float().to(dt)
    allow = ~(mask & ~flags[:, :, None])[:, None].expand(B, heads, Lq, Lk)
    raw, p, _ = attend(q.double(), k.double(), v, scale, None, allow)
    plant_large_v(g, v, p.amax(-2))
    v = v.float().to(dt)
    raw, p, want = attend(q.double(), k.double(), v.double(), scale, None, allow)
    if profile == "masked_spike":                                    # the flagged row sees the spike: it IS that row's largest visible logit
        assert (raw[0, :, 1].argmax(-1) == pos[0]).all() and (p[0, :, 1].amax(-1) > 0.99).all()
    if not (profile == "rising" and Lk <= tile):
        check_reference(raw, allow, want, profile, j // tile)
    else:
        check_reference(raw, allow, want, "falling")
    e32 = None
    if dt == torch.float32:
        e32 = float((attend(q, k, v, scale, None, allow)[2].double() - want).abs().max())
    D = heads * HDM
    pack = lambda t: t.transpose(1, 2).reshape(-1, D)                # noqa: E731  (B, heads, L, hd) -> (B * L, D)
    return dict(q=pack(q), k=pack(k), v=pack(v), vt=v.permute(0, 1, 3, 2).reshape(B * D, Lk), mask=mask.to(torch.uint8), flags=flags.to(torch.uint8),
                want=pack(want), e32=e32)


@pytest.mark.parametrize("profile", ["rising", "falling", "spike", "masked_spike"])
@pytest.mark.parametrize("kind,B,heads,Lq,Lk", MHA)
def test_mha_attention_range(ops, kind, B, heads, Lq, Lk, profile):
    c = mha_case(kind, B, heads, Lq, Lk, profile)
    d, D = ops.device, heads * HDM
    dt = c["q"].dtype
    mask, flags = c["mask"].to(d), c["flags"].to(d)
    if kind == "bf16t":
        qb = torch.zeros(B * Lq, D + 8, dtype=dt)
        kb = torch.zeros(B * Lk, 3 * D, dtype=dt)
        qb[:, 8:] = c["q"]
        kb[:, D:2 * D] = c["k"]
        vt = torch.zeros(B * D, (Lk + 7) // 8 * 8 + 8, dtype=dt)
        vt[:, :Lk] = c["vt"]
        qd, kd = qb.to(d), kb.to(d)
        got = ops.mha_attention_t(qd[:, 8:8 + D], kd[:, D:2 * D], vt.to(d), B, Lq, Lk, heads, mask, flags)
        name = "mha_bf16_mfma_splitkv"
    else:
        o = 3 if kind == "scalar_f32" else 8                          # a 12-byte column offset: not 16-byte aligned -> the per-wave mha_attention_kernel
        qb = torch.zeros(B * Lq, D + 8, dtype=dt)
        kvb = torch.zeros(B * Lk, 2 * D + 4, dtype=dt)
        qb[:, o:o + D] = c["q"]
        kvb[:, :D] = c["k"]
        kvb[:, D + 4:] = c["v"]
        qd, kvd = qb.to(d), kvb.to(d)
        if kind == "scalar_f32":
            assert qd[:, o:o + D].data_ptr() % 16 != 0
        got = ops.mha_attention(qd[:, o:o + D], kvd[:, :D], kvd[:, D + 4:], B, Lq, Lk, heads, mask, flags)
        name = {"f32": "mha_f32_mfma_chunks", "scalar_f32": "mha_scalar_f32", "scalar_bf16": "mha_scalar_bf16"}[kind]
    got = got.cpu()
    err, bar = report(name, f"{Lq}x{Lk}/{profile}", got, c["want"], c["e32"])
    assert torch.isfinite(got.float()).all() and err <= bar
