"""Inputs of the image-session tests (tests/test_11_session_emu.py, tests/test_12_session_gpu.py): N prompts on ONE image."""
import torch

from psalm_amd.synthetic import fix_indices, session_inputs  # noqa: F401


def prefix_cache_vs_one_shot(model, inp):
    """Every layer's K / V of the prefix rows, twice: as the session's prefix pass (one psalm_phi_prefix call where the stage entries are on) leaves
    them in the cache, and as the ONE-SHOT pass over the whole batch (forward_logits on the same prompts, PSALM.llm's op-by-op sequence) leaves
    them -- RoPE'd K in the prefill kernel's workspace (phi_rope_prep_f32_kernel's output), V in the [k|v|q|fc1] GEMM's v columns -- read behind
    each layer's attention call.  Returns (P, [per layer: (K cache (heads, P, 64), V cache (P, hidden), one-shot K (B, heads, P, 64),
    one-shot V (B, P, hidden))]), all on the CPU."""
    import ctypes
    o, cfg = model.ops, model.cfg
    Hd = cfg.hidden_size
    sess = model.encode_image(inp["images"][:1], inp["seg_info"][0])
    model.segment(sess, postprocess=False, **{k: v for k, v in seg_kwargs(inp).items() if k != "is_thing_list"})
    P = sess.prefix_len
    rec = []
    o.lib.psalm_causal_attention_f32_workspace.restype = ctypes.c_long

    def spy(real):
        def run(buf, q_off, k_off, v_off, *rest):
            B, L, heads = rest[-5], rest[-4], rest[-3]
            r = real(buf, q_off, k_off, v_off, *rest)
            Lp = (L + 31) // 32 * 32
            n = B * heads * Lp * 64
            ws = o._ws[("causal_f32_ws", o.lib.psalm_causal_attention_f32_workspace(B, L, heads))]
            kr = ws[4 * n:8 * n].view(torch.float32).view(B, heads, Lp, 64)[:, :, :P].cpu().clone()
            v = buf.view(B, L, -1)[:, :P, v_off:v_off + Hd].cpu().clone()
            rec.append((kr, v))
            return r
        return run

    real = o.causal_attention, o.causal_attention_split
    stages_on = model.c_stages
    o.causal_attention, o.causal_attention_split = spy(real[0]), spy(real[1])
    model.c_stages = False
    try:
        model.forward_logits(**{k: v for k, v in inp.items() if k not in ("is_thing_list", "labels")})
    finally:
        model.c_stages = stages_on
        del o.causal_attention, o.causal_attention_split
    assert len(rec) == cfg.num_layers
    return P, [(kc[:, :P].cpu(), vc.cpu(), kr, v) for (kc, vc), (kr, v) in zip(sess.prefix_cache[1], rec)]


def seg_kwargs(inp):
    return {k: v for k, v in inp.items() if k not in ("images", "labels", "vp_images")}
