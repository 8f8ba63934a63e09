"""RoPE in the [k|v|q|fc1] GEMM's epilogue (psalm_gemm_x3_split_rope) + the attention without its pre-pass (psalm_phi_attention_tables,
psalm_causal_attention_f32_split_prepared) + their use in psalm_phi_forward (PSALM_TUNE_PHI_ROPE_EPILOGUE).

The reference is always the pre-pass path: plain psalm_gemm_x3_split into the fp32 buffer, then psalm_causal_attention_f32_split, whose first
launch (phi_rope_prep_f32_kernel) leaves Qr | Kr | Mk | Tk in the attention workspace.  Everything is compared bit for bit (int32 views: -0 and
+0 differ, NaNs compare by payload).  Shapes: the smallest width the paired 256 x 256 form accepts -- heads 4, hidden 256, intermediate 512.
ops.lib.records / .calls list calls of the C ABI, and psalm_phi_forward is ONE such call: which launches it issues is asked of
psalm_phi_forward_plan (the function psalm_phi_forward itself decides by), and shown by the k / q columns of the fp32 buffer staying unwritten."""
import pytest
import torch

import psalm_amd.hip_ops as H
from ops_backend import ops  # noqa: F401

HEADS, HD, INTER = 4, 256, 512
N1 = 3 * HD + INTER
FORM_256 = "gemm_bf16_glds_kernel<float, 256, 256, 2, 4, 2, false, 32, 4, 2, true, true>"
CASES = [(1, 37), (2, 45), (1, 300)]      # one ragged m-tile, Lp = 64 | a sequence boundary inside a 32-row MFMA tile, Lp != L | two m-tiles, the second partial


def bits(t):
    t = t.cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.dtype == torch.float16 else t)


def rope_tables(L, d):
    inv = 1.0 / (10000.0 ** (torch.arange(0, 32, 2, dtype=torch.float32) / 32))
    emb = torch.cat([torch.arange(L, dtype=torch.float32)[:, None] * inv[None]] * 2, -1)
    return emb.cos().contiguous().to(d), emb.sin().contiguous().to(d)


def bound_par(w1, b1):
    """the 4 bound parameters of psalm_gemm_x3_split for the fc1 rows, floor = the bound of |v| (the attention output shares the row scales)"""
    l1 = lambda w: float(w.abs().double().sum(1).max()) * (1 + 1e-5)
    return torch.tensor([2.0 ** 14 * l1(w1[3 * HD:]), float(b1[3 * HD:].abs().max()), 2.0 ** 14 * l1(w1[HD:2 * HD]), float(b1[HD:2 * HD].abs().max())])


def layer_weights(g, paired=True):
    w1, b1 = torch.randn(N1, HD, generator=g) * 0.2, torch.randn(N1, generator=g)
    par = bound_par(w1, b1)
    if paired:
        perm = torch.cat([torch.arange(3 * HD), 3 * HD + H.Ops.so_pair_perm(INTER)])
        w1, b1 = w1[perm], b1[perm]
    return w1, b1, par


_REF = {}


def gemm_pair(ops, B, L, policy):
    """(reference, RoPE form) of one [k|v|q|fc1] GEMM + attention on the same operands: dicts of CPU tensors"""
    key = (id(ops), B, L, policy)
    if key in _REF:
        return _REF[key]
    d, M, Lp = ops.device, B * L, (L + 31) // 32 * 32
    g = torch.Generator().manual_seed(100 * B + L)
    a = (torch.rand(M, HD, generator=g) * 16 - 8) * torch.exp2(torch.randint(-3, 1, (M, 1), generator=g).float())     # activations up to +-8
    w1, b1, par = layer_weights(g)
    mask = torch.ones(B, L, dtype=torch.uint8)
    mask[-1, L - 3:] = 0
    cos, sin = rope_tables(L, d)
    K2 = HD + INTER
    ws = ops.causal_attention_workspace(B, L, HEADS)
    nq = B * HEADS * Lp * 64
    res = []
    ops.gemm_tile_policy(policy)
    try:
        asp, wsp = ops.split_f16(a.to(d)), ops.split_f16(w1.to(d))
        for rope in (False, True):
            ws.fill_(0xFF)                                    # fp32 view: NaN everywhere
            big = torch.full((M, 3 * HD), 7.0, device=d)
            so = torch.zeros(M, 2 * K2, dtype=torch.float16, device=d)
            inv = torch.full((M,), -1.0, device=d)
            kw = dict(split_col_off=HD, split_col_start=3 * HD, act_col_start=3 * HD, out=big, global_rows=True, paired=True)
            if rope:
                ops.phi_attention_tables(mask.to(d), ws, B, L, HEADS)
                ops.gemm_x3_split(asp, wsp, b1.to(d), H.ACT_GELU_NEW, so, inv, par.to(d), **kw,
                                  rope=dict(ws=ws, cos=cos, sin=sin, q_col=2 * HD, k_col=0, heads=HEADS, B=B, L=L))
                kern = ops.gemm_last_kernel()
                after_gemm = ws.cpu().clone()
                ops.causal_attention_split_prepared(big, HD, so, inv, 0, ws, B, L, HEADS, 64)
            else:
                ops.gemm_x3_split(asp, wsp, b1.to(d), H.ACT_GELU_NEW, so, inv, par.to(d), **kw)
                kern = ops.gemm_last_kernel()
                ops.causal_attention_split(big, 2 * HD, 0, HD, so, inv, 0, cos, sin, mask.to(d), B, L, HEADS, 64, 32)
                after_gemm = None
            wsc = ws.cpu()
            res.append(dict(kern=kern, big=big.cpu(), so=so.cpu(), inv=inv.cpu(), qk=wsc[:8 * nq].view(torch.float32).view(2, B, HEADS, Lp, 64),
                            tables=wsc[8 * nq:8 * nq + B * Lp + B * (Lp // 32)].clone(), after_gemm=after_gemm))
    finally:
        ops.gemm_tile_policy(0)
    _REF[key] = tuple(res)
    return _REF[key]


@pytest.mark.parametrize("B,L", CASES)
def test_gemm_rope_epilogue_bitwise(ops, B, L):
    """Qr, Kr, the v columns of the fp32 buffer, the split fc1 operand and its row scales from the RoPE form == the pre-pass path's, on the
    paired 256 x 256 phased form; the workspace is NaN before: after the tables launch + the GEMM no NaN is left in Qr / Kr, padding rows
    included; the k / q columns of the fp32 buffer are not written any more."""
    ref, new = gemm_pair(ops, B, L, 256)
    assert ref["kern"] == new["kern"] == FORM_256
    Lp = (L + 31) // 32 * 32
    qk = new["after_gemm"][:8 * B * HEADS * Lp * 64].view(torch.float32)
    assert not torch.isnan(qk).any()
    assert torch.equal(bits(new["qk"]), bits(ref["qk"])) and torch.equal(new["tables"], ref["tables"])
    assert (ref["qk"][:, :, :, :L].abs() > 0).any() and (ref["qk"][:, :, :, L:] == 0).all()
    assert torch.equal(bits(new["big"][:, HD:2 * HD]), bits(ref["big"][:, HD:2 * HD]))
    assert (new["big"][:, :HD] == 7.0).all() and (new["big"][:, 2 * HD:] == 7.0).all() and (ref["big"] != 7.0).all()
    assert torch.equal(bits(new["inv"]), bits(ref["inv"]))
    assert torch.equal(bits(new["so"]), bits(ref["so"])) and (ref["so"][:, :HD] != 0).any() and (ref["so"][:, HD:HD + INTER] != 0).any()


@pytest.mark.parametrize("policy", [128, 64, 0])
def test_gemm_rope_epilogue_other_paired_forms(ops, policy):
    """the same through the other paired instantiations -- 128 x 128, 64 x 128 tiles and the automatic selection -- which carry the same
    epilogue code (B = 2, L = 45: the sequence boundary inside a matrix tile)"""
    ref, new = gemm_pair(ops, 2, 45, policy)
    assert ref["kern"] == new["kern"] and ref["kern"].endswith("true, true>")
    assert torch.equal(bits(new["qk"]), bits(ref["qk"])) and torch.equal(new["tables"], ref["tables"])
    assert torch.equal(bits(new["big"][:, HD:2 * HD]), bits(ref["big"][:, HD:2 * HD])) and (new["big"][:, :HD] == 7.0).all()
    assert torch.equal(bits(new["inv"]), bits(ref["inv"])) and torch.equal(bits(new["so"]), bits(ref["so"]))


@pytest.mark.parametrize("mask_kind", ["all_valid", "hole_in_middle_tile", "tail_masked"])
def test_attention_tables_bitwise(ops, mask_kind):
    """Mk / Tk of psalm_phi_attention_tables == the pre-pass's; the padding rows of Qr / Kr are zeroed, nothing else of them is touched"""
    B, L, Lp, d = 2, 70, 96, ops.device
    mask = torch.ones(B, L, dtype=torch.uint8)
    if mask_kind == "hole_in_middle_tile":
        mask[0, 40:45] = 0
        mask[1, 33] = 0
    elif mask_kind == "tail_masked":
        mask[0, 60:] = 0
        mask[1, 69:] = 0
    g = torch.Generator().manual_seed(7)
    buf = (torch.randn(B * L, 3 * HD, generator=g)).to(d)
    cos, sin = rope_tables(L, d)
    ws = ops.causal_attention_workspace(B, L, HEADS)
    nq, nt = B * HEADS * Lp * 64, B * Lp + B * (Lp // 32)
    ws.fill_(0xFF)
    ops.causal_attention(buf, 2 * HD, 0, HD, torch.empty(B * L, HD, device=d), 0, cos, sin, mask.to(d), B, L, HEADS, 64, 32)
    want = ws.cpu()[8 * nq:8 * nq + nt].clone()
    ws.fill_(0xFF)
    ops.phi_attention_tables(mask.to(d), ws, B, L, HEADS)
    got = ws.cpu()
    assert torch.equal(got[8 * nq:8 * nq + nt], want)
    assert want[:B * Lp].view(B, Lp)[:, :L].eq(mask).all() and (want[:B * Lp].view(B, Lp)[:, L:] == 0).all()
    qk = got[:8 * nq].view(torch.float32).view(2, B, HEADS, Lp, 64)
    assert (qk[:, :, :, L:] == 0).all() and torch.isnan(qk[:, :, :, :L]).all()


def phi_descriptor(ops, paired, seed=5):
    g, d, layers = torch.Generator().manual_seed(seed), ops.device, []
    for _ in range(2):
        w1, b1, par = layer_weights(g, paired)
        w2, b2 = torch.randn(HD, HD + INTER, generator=g) * 0.05, torch.randn(HD, generator=g) * 0.1
        layers.append(dict(w1=ops.split_f16(w1.to(d)), b1=b1.to(d), w2=ops.split_f16(w2.to(d)), b2=b2.to(d),
                           ln_g=(1 + 0.1 * torch.randn(HD, generator=g)).to(d), ln_b=(0.1 * torch.randn(HD, generator=g)).to(d),
                           bnd=par.to(d), paired=paired))
    return ops.phi_desc(layers, HD, INTER, HEADS, 64, 32, 1e-5, torch.ones(HD, device=d), torch.zeros(HD, device=d))


def phi_both_switches(ops, desc, B, L, policy):
    d = ops.device
    g = torch.Generator().manual_seed(B + L)
    embeds = torch.randn(B * L, HD, generator=g).to(d)
    mask = torch.ones(B, L, dtype=torch.uint8)
    mask[-1, L - 2:] = 0
    cos, sin = rope_tables(L, d)
    out = {}
    ops.gemm_tile_policy(policy)
    try:
        for sw in (0, 1):
            ops.set_tuning(H.Ops.TUNE_PHI_ROPE_EPILOGUE, sw)
            out[sw] = (ops.phi_forward_plan(desc, B, L), ops.phi_forward(desc, embeds, mask.to(d), cos, sin, B, L).cpu())
    finally:
        ops.set_tuning(H.Ops.TUNE_PHI_ROPE_EPILOGUE, 1)
        ops.gemm_tile_policy(0)
    return out


@pytest.mark.parametrize("B,L,policy", [(1, 37, 256), (2, 45, 256)])
def test_phi_forward_switch_bitwise(ops, B, L, policy):
    """a 2-layer psalm_phi_forward: identical hidden states with the switch 0 (five launches per layer, the pre-pass among them) and 1 (four
    launches per layer + one tables launch in front); the switch defaults to 1"""
    assert ops.get_tuning(H.Ops.TUNE_PHI_ROPE_EPILOGUE) == 1
    out = phi_both_switches(ops, phi_descriptor(ops, True), B, L, policy)
    assert out[0][0] == (False, 5, 1) and out[1][0] == (True, 4, 2)
    assert torch.isfinite(out[0][1]).all() and out[0][1].abs().max() > 0.1
    assert torch.equal(bits(out[1][1]), bits(out[0][1]))


@pytest.mark.parametrize("why", ["unpaired_layers", "short_sequences"])
def test_phi_forward_fallback(ops, why):
    """what the RoPE form does not cover -- fc1 rows not in the paired layout (the kernels then selected have no RoPE epilogue), B > 1 with
    L < 32 -- runs the pre-pass sequence under the switch's default: no error, the same bits as with the switch off"""
    B, L = (1, 37) if why == "unpaired_layers" else (2, 20)
    out = phi_both_switches(ops, phi_descriptor(ops, why != "unpaired_layers"), B, L, 0)
    assert out[0][0] == out[1][0] == (False, 5, 1)
    assert torch.isfinite(out[1][1]).all() and torch.equal(bits(out[1][1]), bits(out[0][1]))
