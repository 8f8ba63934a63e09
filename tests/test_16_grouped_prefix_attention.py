"""Grouped prefix form of the Phi attention (PSALM.segment_many: every prompt names its own prefix cache and prefix length through a device
table): psalm_causal_attention_f32_prefix_grouped[_split] against the ungrouped kernel (bitwise) and against a plain torch restatement.  Runs on
the host emulation of the kernels here and on the real GPU under `-m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

from grouped_util import HD, ROT, attention_case, attention_caches
from ops_backend import ops  # noqa: F401
from psalm_amd.hip_ops import PsalmHipError


def tol(want):                                     # tests/test_10_prefix_attention.py tol
    return 3e-5 * want.abs().max()


A = dict(heads=2, Ps=[40, 64, 1], groups=[0, 1, 2], S=70)          # three caches; npt & 3 = 2, 2, 1: the first suffix wave differs between prompts
B = dict(heads=4, Ps=[130, 130, 33, 97], groups=[0, 0, 1, 2], S=20)  # prompts 0, 1 share a cache; heads * N % 8 == 0: XCD placement active
C = dict(heads=1, Ps=[1], groups=[0], S=100)                       # the degenerate single group


def _grouped(ops, c, caches, o_off=0, P_max=None):
    d, H, N, S = ops.device, c["H"], c["N"], c["S"]
    table = ops.prefix_ref_table(caches, c["groups"])
    assert table.shape == (1, N) and table.dtype.itemsize == 32
    out = torch.zeros(N * S, H + o_off, device=d)
    ops.causal_attention_prefix_grouped(c["suf"].to(d), 0, H + 8, 2 * H + 16, table[0], out, o_off, c["cos"].to(d), c["sin"].to(d),
                                        c["mask"].to(d), N, S, max(c["Ps"]) if P_max is None else P_max, c["heads"], HD, ROT)
    return out


def _ungrouped(ops, c, caches, n, S=None, rows=None, mask=None):
    """prompt n alone through the ungrouped entry: N = 1, its cache, its P"""
    d, H = ops.device, c["H"]
    S = c["S"] if S is None else S
    kc, vc = caches[c["groups"][n]][1][0]
    suf = c["suf"][n * c["S"]:n * c["S"] + S] if rows is None else rows
    mask = c["mask"][n:n + 1, :S] if mask is None else mask
    out = torch.zeros(S, H, device=d)
    ops.causal_attention_prefix(suf.contiguous().to(d), 0, H + 8, 2 * H + 16, kc, vc, out, 0, c["cos"].to(d), c["sin"].to(d),
                                mask.contiguous().to(d), 1, S, c["Ps"][n], c["heads"], HD, ROT)
    return out


@pytest.mark.parametrize("shape", [A, B, C], ids=["three_caches", "shared_cache_xcd", "single"])
def test_grouped_is_bitwise_the_ungrouped_kernel_per_prompt(ops, shape):
    """A block's tile list, wave dealing and merge depend only on (P_n, qt) and on that prompt's rows and mask, and its arithmetic is the ungrouped
    kernel's word for word: equal bits, not a tolerance."""
    c = attention_case(**shape)
    caches = attention_caches(ops, c)
    got = _grouped(ops, c, caches)
    assert torch.isfinite(got).all()
    S = c["S"]
    for n in range(c["N"]):
        assert torch.equal(got[n * S:(n + 1) * S], _ungrouped(ops, c, caches, n)), f"prompt {n}"


def test_grouped_prompts_of_different_real_lengths(ops):
    """S = 70 with prompt 1's keys >= 33 masked: its rows 0..32 == an ungrouped call with S = 33 on the same 33 rows (masked keys get probability
    exactly 0 and every V row is finite, so the extra tiles add zeros)."""
    c = attention_case(mask_from=33, **A)
    caches = attention_caches(ops, c)
    got = _grouped(ops, c, caches)
    S = c["S"]
    ref = _ungrouped(ops, c, caches, 1, S=33, mask=torch.ones(1, 33, dtype=torch.uint8))
    assert torch.equal(got[S:S + 33], ref)


def test_grouped_vs_torch(ops):
    c = attention_case(**B)
    got = _grouped(ops, c, attention_caches(ops, c)).cpu()
    err = (got - c["want"]).abs().max()
    print(f"grouped prefix attention (heads={c['heads']}, P={c['Ps']}, S={c['S']}): max err {err:.3e}, bound {tol(c['want']):.3e}")
    assert torch.isfinite(got).all()
    assert err <= tol(c["want"])


def test_grouped_split_output(ops):
    """the _grouped_split entry == the _grouped entry followed by a split under the given per-row scales (test_prefix_attention_split_output's assertions)"""
    c = attention_case(**B)
    d, Hh, N, S = ops.device, c["H"], c["N"], c["S"]
    caches = attention_caches(ops, c)
    ref = _grouped(ops, c, caches).cpu()
    g = torch.Generator().manual_seed(17)
    vmax = torch.stack([c["suf"][:, 2 * Hh + 16:].abs().max()] + [p[:, 2 * Hh + 16:].abs().max() for p in c["pre"]]).max()
    inv = torch.exp2(torch.ceil(torch.log2(vmax)) - 12 + torch.randint(0, 4, (N * S,), generator=g).float())    # |v| / inv < 2^13
    off = 64
    Kp = (off + Hh + 63) // 64 * 64 + 64
    so = torch.zeros(N * S, 2 * Kp, dtype=torch.float16, device=d)
    ops.causal_attention_prefix_grouped_split(c["suf"].to(d), 0, Hh + 8, 2 * Hh + 16, ops.prefix_ref_table(caches, c["groups"])[0], so, inv.to(d),
                                              off, c["cos"].to(d), c["sin"].to(d), c["mask"].to(d), N, S, max(c["Ps"]), c["heads"], HD, ROT)
    so = so.cpu()
    hi, lo = so[:, off:off + Hh].double(), so[:, Kp + off:Kp + off + Hh].double()
    rec = (hi + lo) * inv.double()[:, None]
    assert ((rec - ref.double()).abs() <= 2.0 ** -21 * ref.abs().double() + 2.0 ** -24 * inv.double()[:, None]).all()
    assert hi.abs().max() < 2.0 ** 13
    mask = torch.ones(2 * Kp, dtype=torch.bool)
    mask[off:off + Hh] = False
    mask[Kp + off:Kp + off + Hh] = False
    assert (so[:, mask] == 0).all()


def test_grouped_reads_only_and_rejects_bad_tables(ops):
    c = attention_case(**A)
    d, H, N, S = ops.device, c["H"], c["N"], c["S"]
    caches = attention_caches(ops, c)
    before = [(kc.clone(), vc.clone()) for _, [(kc, vc)] in caches]
    out = _grouped(ops, c, caches, o_off=32)
    assert out[:, :32].abs().max() == 0                           # padding columns of the output buffer untouched
    assert (out[:, 32:].cpu() - c["want"]).abs().max() <= tol(c["want"])
    for (_, [(kc, vc)]), (kc0, vc0), P in zip(caches, before, c["gP"]):
        assert torch.equal(kc, kc0) and torch.equal(vc, vc0)      # the prefix caches are read only
        assert (kc[:, P:] == 0).all()                             # ... and their padding rows are zeros
    # what the host can know: the binding checks the host copy of the table it uploads ...
    table = ops.prefix_ref_table(caches, c["groups"])[0]
    args = (c["cos"].to(d), c["sin"].to(d), c["mask"].to(d), N, S)
    fresh = torch.zeros(N * S, H, device=d)
    zero = table.copy()
    zero["P"][1] = 0
    with pytest.raises(PsalmHipError, match="P_max"):
        ops.causal_attention_prefix_grouped(c["suf"].to(d), 0, H + 8, 2 * H + 16, zero, fresh, 0, *args, 64, c["heads"], HD, ROT)
    with pytest.raises(PsalmHipError, match="P_max"):             # P_max below a table P
        ops.causal_attention_prefix_grouped(c["suf"].to(d), 0, H + 8, 2 * H + 16, table, fresh, 0, *args[:2], c["mask"].to(d), N, S, 63, c["heads"],
                                            HD, ROT)
    # ... and the entry itself a null table and P_max < 1: non-zero with psalm_last_error()
    ops.lib.psalm_last_error.restype = ctypes.c_char_p
    with pytest.raises(PsalmHipError, match="null table"):
        ops.causal_attention_prefix_grouped(c["suf"].to(d), 0, H + 8, 2 * H + 16, None, fresh, 0, *args, 64, c["heads"], HD, ROT)
    assert b"psalm_causal_attention_f32_prefix_grouped" in ops.lib.psalm_last_error()
    dev = torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).reshape(-1).copy()).to(d)
    cosl = torch.cat((c["cos"], c["cos"])).to(d)                  # (long enough for the binding's own table-length check at any P_max)
    with pytest.raises(PsalmHipError, match="P_max < 1"):
        ops.causal_attention_prefix_grouped(c["suf"].to(d), 0, H + 8, 2 * H + 16, dev, fresh, 0, cosl, cosl, c["mask"].to(d), N, S, 0, c["heads"], HD, ROT)
    assert fresh.abs().max() == 0                                 # nothing ran
