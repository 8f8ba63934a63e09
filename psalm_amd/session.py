"""Image sessions of `psalm_amd.model.PSALM`: encode an image once (`encode_image` -> ImageSession), then run many prompts on it (`segment`), or prompts
on several encoded images in one Phi pass (`segment_many`).  A mixin that PSALM inherits: everything here runs on the model's own weights, kernels
and caches (`self.ops`, `self.w`, `self._cache`) and calls its one-shot building blocks -- `_splice_plan`, `_llm_setup` / `_llm_layers`,
`_decoder_embeddings`, `_prompt_operands`, `predictor`, `_postprocess`, `_finalize`.

One pipeline serves both fronts (`_segment_requests`); they differ in how the suffix rows attend the prefix -- `segment` against its session's own
cache, `segment_many` through the table of cache references of the grouped kernels -- and in the texts of their errors.
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import torch

from .config import IMAGE_TOKEN_INDEX, REGION_TOKEN_INDEX


# (The two default samplers are keyword defaults of `segment` / `segment_many` and of model.py's one-shot entry points: they live here, the module
#  that imports nothing from the other, and model.py re-exports them.)
def default_region_point_sampler(nonzero: torch.Tensor, n: int) -> torch.Tensor:
    """Row indices into `nonzero` (context_cluster.py:31-40 rand_sample_repeat; global torch CPU RNG, same call order)."""
    m = nonzero.shape[0]
    if m < n:
        return torch.cat((torch.arange(m), torch.randint(0, m, (n - m,))))
    if m == n:
        return torch.arange(m)
    return torch.randperm(m)[:n]


def default_region_index_sampler(m: int, n: int) -> torch.Tensor:
    """`default_region_point_sampler` (context_cluster.py:31-40 rand_sample_repeat) with the number of non-zero pixels as its argument: row indices
    into a `nonzero()` of m rows.  The same global-RNG calls in the same order."""
    m = int(m)
    if m < n:
        return torch.cat((torch.arange(m), torch.randint(0, m, (n - m,))))
    if m == n:
        return torch.arange(m)
    return torch.randperm(m)[:n]


class ImageSession:
    """What `PSALM.encode_image` keeps on the device for one image, so that `PSALM.segment` runs only the prompt-dependent part of the model:
    the four Swin levels (`feats`), the projector's image tokens, the pixel decoder's outputs (`mask_features`, `multi_scale_features` + sizes),
    the predictor's K / V front per region count (built lazily) and the Phi prefix cache -- RoPE'd K and V of the prompt-independent first P rows
    (system text + image tokens) of every layer, built on the first `segment` call and reused while the leading text ids stay the same
    (`prefix_builds` / `prefix_hits` count both).  Belongs to the model (or replica) that made it."""

    def __init__(self, model, images, seg_info, feats, image_tokens, n_img, pd):
        self.model, self.version = model, model._weights_version
        self.images, self.seg_info = images, seg_info
        self.feats, self.image_tokens, self.n_img = feats, image_tokens, n_img
        self.mask_features, self.multi_scale_features, self.shapes, self.mask_features_size = pd
        self.kv = {}                              # region count -> predictor K / V handle (session-owned workspace)
        self.prefix_key = None                    # tuple of the leading text ids the cache below was built for
        self.prefix_len = 0                       # P
        self.prefix_cache = None                  # (buffer, per-layer (K (heads, ceil32 P, 64), V (P, hidden)) views)
        self.prefix_builds = self.prefix_hits = 0
        self.region_tables = None                 # `regions=` prompts: (geometry, row table, column table) of psalm_mask_resize_nearest_pad on the device

    def nbytes(self) -> int:
        """device bytes held: vision tensors + K / V fronts + prefix cache (2 * layers * P * hidden * 4 up to padding)"""
        ts = [t for t, _, _ in self.feats] + [self.image_tokens, self.mask_features] + list(self.multi_scale_features)
        n = sum(t.numel() * t.element_size() for t in ts) + sum(h[0][0].numel() for h in self.kv.values() if h is not None)
        return n + (self.prefix_cache[0].numel() if self.prefix_cache is not None else 0)


class SessionMixin:
    """`encode_image`, `segment`, `segment_many` and what only they use, as methods of PSALM (see the module docstring)."""

    def _session_mode_check(self):
        if self.precision == "bf16":
            raise NotImplementedError("image sessions: precision 'bf16' is a side line with its own attention kernels (f16x3 / fp32 only)")
        if self.llm_products != 3:
            raise NotImplementedError("image sessions: llm_products=1 is a side mode of the one-shot path (llm_products=3 only)")

    @torch.no_grad()
    def encode_image(self, images, seg_info=None) -> "ImageSession":
        """Everything of eval_seg that does not read the prompt, for ONE image ((1, 3, H, W) or (3, H, W), pre-processed as for eval_seg; `seg_info`: its
        geometry entry -- a dict, or a list holding it): Swin, projector, pixel decoder.  Returns the ImageSession `segment` takes."""
        self._session_mode_check()
        if images.dim() == 3:
            images = images[None]
        if images.dim() != 4 or images.shape[0] != 1:
            raise ValueError("encode_image: one image, (1, 3, H, W) or (3, H, W)")
        if isinstance(seg_info, (list, tuple)):
            if len(seg_info) != 1:
                raise ValueError("encode_image: seg_info of one image")
            seg_info = seg_info[0]
        images = images.to(self.device, torch.float32).contiguous()
        feats = self.swin(images)
        res5, h5, w5 = feats[3]
        img_tok, n_img = self.projector(res5, 1, h5, w5)
        pd = self.pixel_decoder([(tok, h, w_) for tok, h, w_ in feats])
        return ImageSession(self, images, seg_info, feats, img_tok, n_img, pd)

    def _session_kv(self, session, n_reg):
        """the predictor's K / V front for this region count, in a workspace the session owns (built on first use)"""
        if n_reg not in session.kv:
            mf, ms, shapes, mfs = session.mask_features, session.multi_scale_features, session.shapes, session.mask_features_size
            kv = None
            if self.kv_side and self._predictor_native_ok(mf):
                desc, prpos = self._predictor_desc(shapes)
                cont = lambda t: t if t.is_contiguous() else t.contiguous()       # noqa: E731
                ms_c, mf_c = [cont(t) for t in ms], cont(mf)
                kv = (self.ops.predictor_kv(desc, ms_c, shapes, prpos, mf_c, mfs, n_reg, slot=0, own=True), ms_c, mf_c)
            session.kv[n_reg] = kv
        return session.kv[n_reg]

    def _session_plan(self, session, input_ids, attention_mask, class_name_ids, cls_indices, token_refer_id, n_regions, want_cls, want_refer):
        """The splice plan of N prompts on the session's image, cut at P = the row just past the last image row: the shared prefix's (sid, srow) and
        its key (the leading text ids), and the suffix plan -- (N, S) arrays with S bucketed by `len_bucket` as `_bucketed` does for L, row sets
        re-based from absolute to suffix positions."""
        ids = input_ids.cpu().numpy().astype(np.int64)
        N, T = ids.shape
        n_img = session.n_img
        t_img = []
        for b in range(N):
            pos = np.flatnonzero(ids[b] == IMAGE_TOKEN_INDEX)
            if pos.shape[0] != 1:
                raise ValueError(f"segment: prompt {b} holds {pos.shape[0]} <image> tokens, a session prompt has exactly one")
            if (ids[b, :pos[0]] < 0).any():
                raise ValueError(f"segment: prompt {b} has a special token at position {int(np.flatnonzero(ids[b, :pos[0]] < 0)[0])}, before <image>: "
                                 "the shared prefix is text + <image>")
            t_img.append(int(pos[0]))
        for b in range(1, N):
            n = min(t_img[0], t_img[b]) + 1
            diff = np.flatnonzero(ids[b, :n] != ids[0, :n])
            if diff.shape[0] or t_img[b] != t_img[0]:
                at = int(diff[0]) if diff.shape[0] else n
                raise ValueError(f"segment: prompt {b} differs from prompt 0 at token position {at}; all prompts of a call must share the rows up to "
                                 "and including <image>")
        key = tuple(int(v) for v in ids[0, :t_img[0]])
        P = t_img[0] + n_img
        plan = self._splice_plan(input_ids, attention_mask, n_img, class_name_ids, cls_indices, token_refer_id, n_regions, want_cls, want_refer)
        L = plan["L"]
        if not plan["kmask"][:, :P].all():
            raise ValueError("segment: the attention mask hides a row of the shared prefix (prefix rows are always real)")
        S = L - P
        if S < 1:
            raise ValueError("segment: nothing follows <image>")
        q = max(int(self.len_bucket or 0), 1)
        Sb = (S + q - 1) // q * q
        sid = np.full((N, Sb), -1, np.int32)
        srow = np.zeros((N, Sb), np.int32)
        kmask = np.zeros((N, Sb), np.uint8)
        sid[:, :S], srow[:, :S], kmask[:, :S] = plan["sid"][:, P:], plan["srow"][:, P:], plan["kmask"][:, P:]
        psrow = plan["srow"][0, :P].copy()
        psrow[plan["sid"][0, :P] == 1] %= n_img                   # (one image: its tokens are rows 0 .. n_img-1 whatever the prompt index)
        out = {"P": P, "S": Sb, "S_real": S, "lens": [l_ - P for l_ in plan["lens"]], "key": key, "n_cls": plan["n_cls"],
               "prefix": (plan["sid"][0, :P].copy(), psrow), "sid": sid, "srow": srow, "kmask": kmask}
        for name in ("seg", "cls", "refer", "region"):
            if plan[name] is None:
                out[name] = None
                continue
            off, rows = plan[name]
            r64 = rows.astype(np.int64)
            assert (r64 % L >= P).all(), "row sets live behind the prefix"
            rows = (r64 // L * Sb + r64 % L - P).astype(np.int32)
            if name != "seg" and q > 1:
                n = (rows.shape[0] + q - 1) // q * q
                rows = np.concatenate((rows, np.zeros(max(n, q) - rows.shape[0], np.int32)))
            out[name] = (off, rows)
        return out

    def _llm_session(self, embeds, key_mask, B, L, P, cache, suffix: bool, refs=None):
        """PSALM.llm cut behind the prompt-independent prefix.  suffix = False: the P prefix rows (B = 1, L = P), every layer's RoPE'd K and its V go
        into `cache` (Ops.phi_prefix_cache), the last layer stops behind its [k|v|q|fc1] GEMM; returns None.  suffix = True: the B * L suffix rows
        at positions P .., attention through the prefix kernel against `cache`; returns the final-LayerNorm hidden states (B*L, hidden).
        One native call each (psalm_phi_prefix / psalm_phi_suffix) under the conditions of PSALM.llm's stage-level call, else PSALM._llm_layers with
        this pass's attention step -- same launches, same bits (tests/test_11_session_emu.py).
        refs (suffix only; `segment_many`): (device bytes, host array) of the (num_layers, B) psalm_prefix_ref table -- prompt b attends the cache and
        prefix length its entries name, P is the largest of them and `cache` is not read; attention through the grouped prefix kernel
        (psalm_phi_suffix_grouped, or the grouped ops as the attention step).  Off by default: the ungrouped path is untouched."""
        o, cfg = self.ops, self.cfg
        if cfg.head_dim != 64 or cfg.rotary_dim != 32:
            raise NotImplementedError("image sessions: the prefix attention kernel is built for head_dim 64 / rotary dim 32 (Phi-1.5)")
        cos, sin = self._rope(P + L if suffix else P)
        buf, views = cache if refs is None else (None, None)
        if refs is not None:
            assert suffix, "a prefix pass writes one cache"
            rdev, rhost = refs
        desc, state = self._llm_setup(embeds, key_mask)
        if desc is not None:
            if refs is not None:
                return o.phi_suffix_grouped(desc, embeds, key_mask, cos, sin, B, L, rdev, P, table=rhost)
            if suffix:
                return o.phi_suffix(desc, embeds, key_mask, cos, sin, B, L, P, buf)
            o.phi_prefix(desc, embeds, key_mask, cos, sin, P, buf)
            return None
        Hd, nh, hd, rd = cfg.hidden_size, cfg.num_heads, cfg.head_dim, cfg.rotary_dim
        if refs is not None:
            def attend(i, split, big, *out):
                op = o.causal_attention_prefix_grouped_split if split else o.causal_attention_prefix_grouped
                op(big, 2 * Hd, 0, Hd, rdev[32 * B * i:32 * B * (i + 1)], *out, cos, sin, key_mask, B, L, P, nh, hd, rd, table=rhost[i])
        elif suffix:
            def attend(i, split, big, *out):
                op = o.causal_attention_prefix_split if split else o.causal_attention_prefix
                op(big, 2 * Hd, 0, Hd, *views[i], *out, cos, sin, key_mask, B, L, P, nh, hd, rd)
        else:
            one_shot = self._llm_attend(cos, sin, key_mask, B, L)

            def attend(i, split, big, *out):
                o.phi_prefix_kv_store(big, 0, Hd, cos, sin, *views[i], P, nh, hd, rd)
                if i == cfg.num_layers - 1:
                    return True                           # (the prefix rows' own hidden states are never read: the pass ends here)
                one_shot(i, split, big, *out)
        return self._llm_layers(embeds, *state, attend)

    def _session_prefix(self, session, sp):
        """the session's Phi prefix cache for this call's leading text ids: reused when the key matches, (re)built otherwise"""
        o, w, cfg = self.ops, self.w, self.cfg
        if session.prefix_cache is not None and session.prefix_key == sp["key"] and session.prefix_len == sp["P"]:
            session.prefix_hits += 1
            return session.prefix_cache
        P = sp["P"]
        psid, psrow = sp["prefix"]
        cache = session.prefix_cache
        session.prefix_key = None                 # (the buffer is rebuilt in place: not a hit for the old text if the pass below raises midway)
        if cache is None or session.prefix_len != P:
            cache = o.phi_prefix_cache(cfg.hidden_size, cfg.num_heads, P, cfg.num_layers)
        embeds = o.gather_rows([w["embed"], session.image_tokens, w["seg_query"], None], self._dev_i32(psid), self._dev_i32(psrow), cfg.hidden_size,
                               out_dtype=torch.float32)
        ones = torch.ones(1, P, dtype=torch.uint8, device=self.device)
        self._llm_session(embeds, ones, 1, P, P, cache, suffix=False)
        session.prefix_cache, session.prefix_key, session.prefix_len = cache, sp["key"], P
        session.prefix_builds += 1
        return cache

    # The mask decoder over the prompts of a session: one native pass over B * Q query rows against the session's one K / V front
    # (psalm_predictor_forward_batched) in place of B `predictor` calls.  Each prompt's words are those of its own call, so the switch changes time only.
    batch_decoder = True
    decoder_batch_max = 8            # prompts per pass: scratch + outputs hold ~2 * B * Q * H2*W2 * 4 bytes of mask logits (1024^2: ~52 MB per prompt)

    def _decode_batched(self, session, prompts):
        """`predictor`'s result dicts for the prompts of ONE session -- prompts: a list of (seg_query (Q, D), SEG_emb, class_emb, region_emb) as the
        per-prompt loop passes them -- through the batched decoder, in chunks of `decoder_batch_max`; None when the per-prompt loop must run: fewer
        than two prompts, `batch_decoder` off, or a prompt outside the native per-prompt path's conditions."""
        o, cfg = self.ops, self.cfg
        n = len(prompts)
        step = int(self.decoder_batch_max)
        if n < 2 or not self.batch_decoder or step < 2:
            return None
        mf, shapes, mfs = session.mask_features, session.shapes, session.mask_features_size
        if not self._predictor_native_ok(mf):
            return None
        Q, D = cfg.md_queries, cfg.md_hidden
        for sq, se, ce, re in prompts:
            if sq.dtype != torch.float32 or sq.data_ptr() % 16 or not sq.is_contiguous():
                return None
            if any(e is not None and (e.dtype != torch.float32 or e.data_ptr() % 16 or not e.is_contiguous()) for e in (se, ce, re)):
                return None
            if (re is not None and re.shape[0] > 192) or any(e is not None and e.shape[0] > 8192 for e in (se, ce)):
                return None                                       # (outside the exact-fp32 skinny kernel's range: the per-prompt call takes another kernel)
        kinds = [tuple(e is not None for e in p[1:]) for p in prompts]
        if len(set(kinds)) != 1:
            return None
        kv = self._session_kv(session, int(prompts[0][3].shape[0]) if prompts[0][3] is not None else 0)
        if kv is None:
            return None
        handle, _, mf_c = kv
        desc, _ = self._predictor_desc(shapes)
        H2, W2 = mfs

        def rows(pieces):                                         # consecutive slices of one tensor stay a view; others are packed by stream copies
            if all(a.data_ptr() + a.numel() * 4 == b_.data_ptr() and a.untyped_storage().data_ptr() == b_.untyped_storage().data_ptr()
                   for a, b_ in zip(pieces, pieces[1:])):
                return pieces[0].as_strided((sum(int(t.shape[0]) for t in pieces), D), (D, 1))
            out = o.empty(sum(int(t.shape[0]) for t in pieces), D)
            r0 = 0
            for t in pieces:
                if t.shape[0]:
                    o.copy_(out[r0:r0 + t.shape[0]], t)
                r0 += int(t.shape[0])
            return out

        def own(t):                                               # a prompt's block of the packed logits, 16-byte aligned as a per-prompt call's tensor is
            if t.data_ptr() % 16 == 0:
                return t
            return o.copy_(o.empty(*t.shape), t)

        outs = []
        for c0 in range(0, n, step):
            chunk = prompts[c0:c0 + step]
            B = len(chunk)
            if B == 1:                                            # (a trailing chunk of one prompt: the per-prompt call, the same words)
                sq, se, ce, re = chunk[0]
                outs.append(self.predictor(session.multi_scale_features, shapes, mf, mfs, sq, se, ce, re,
                                           kv=self._session_kv(session, int(re.shape[0]) if re is not None else 0)))
                continue
            has_s, has_c, has_r = kinds[0]
            cnt = lambda k: [int(p[k].shape[0]) for p in chunk]  # noqa: E731
            masks, cls_l, seg_l, reg_l = o.predictor_forward_batched(
                desc, shapes, handle, mf_c, mfs, rows([p[0] for p in chunk]),
                class_emb=rows([p[2] for p in chunk]) if has_c else None, cls_counts=cnt(2) if has_c else None,
                seg_emb=rows([p[1] for p in chunk]) if has_s else None, seg_counts=cnt(1) if has_s else None,
                region_emb=rows([p[3] for p in chunk]) if has_r else None, reg_counts=cnt(3) if has_r else None)
            oc = os_ = or_ = 0
            for b, (sq, se, ce, re) in enumerate(chunk):
                r = {"pred_masks": masks[b * Q:(b + 1) * Q].view(Q, H2, W2), "pred_class_name_logits": None, "pred_SEG_logits": None,
                     "pred_region_logits": None}
                if has_c:
                    k = int(ce.shape[0])
                    r["pred_class_name_logits"] = own(cls_l[Q * oc:Q * (oc + k)].view(Q, k))
                    oc += k
                if has_s:
                    k = int(se.shape[0])
                    r["pred_SEG_logits"] = own(seg_l[Q * os_:Q * (os_ + k)].view(Q, k))
                    os_ += k
                if has_r:
                    k = int(re.shape[0])
                    r["pred_region_logits"] = own(reg_l[Q * or_:Q * (or_ + k)].view(k, Q))
                    or_ += k
                outs.append(r)
        return outs

    # ---- region prompts given as geometry (`regions=` of segment / segment_many): the dataset mapper's host preparation of a click -- draw the prompt,
    # enhance_with_circles, apply_segmentation, nonzero() (coco_instance_mapper.py:233-252, context_cluster.py:345-356) -- on the device.  The host
    # validates and packs a primitive table; psalm_mask_rasterize / psalm_mask_dilate_disc / psalm_mask_resize_nearest_pad make the (S, S) region masks
    # the host path would have uploaded; ONE read-back brings the R pixel totals the sampler needs; psalm_mask_select_points turns its ranks into the
    # points `region_points` would have computed, bit for bit.
    REGION_PROMPT_KEYS = ("points", "scribble", "box", "mask", "rle", "polygon")
    REGION_PROMPT_RADIUS = {"points": 10, "scribble": 5}              # coco_instance_mapper.py:247-250
    REGION_PROMPT_MAX_RADIUS = 16
    REGION_POLYGON_MAX_VERTICES = 1 << 20                             # per call of _region_prompt_plan, all polygon prompts together

    def _region_prompt_plan(self, session, input_ids, seg_info, regions, tag="", transforms=None, canvas=None):
        """Host side of `regions=` for the N prompts of one session: validation (ValueError naming prompt and region) and the arrays that travel in
        the call's blob under names ending in `tag` -- the primitive table (n, 6) int32, the radii (R) int32 (-1: not dilated), host mask prompts,
        the polygon prompts' ring (P, 4) and vertex (V, 2) tables in psalm_mask_fill_polygons' layout, the all-zero image index of region_pool.
        R = all regions of the N prompts, prompt by prompt.  Without a session (`session=None`, the video tracker): the image's geometry as
        `transforms` (its resize / pad record) and `canvas` (the (H, W) of the model's input)."""
        from .preprocess import rle_to_mask
        if self.seg_task != "region":
            raise ValueError(f"regions are prompts of the region task (this model's seg_task = {self.seg_task!r})")
        if session is not None:
            transforms = session.seg_info.get("transforms") if isinstance(session.seg_info, dict) else None
            canvas = (session.images.shape[2], session.images.shape[3])
        tr, whose = transforms, "session" if session is not None else "frame"
        if tr is None:
            raise ValueError("regions need the session's seg_info['transforms'] (the resize / pad record of the image: encode_image(images, seg_info))")
        h, w, nh, nw = [int(v) for v in tr["resize"]]
        ph, pw = [int(v) for v in tr["pad"]]
        Hi, Wi = int(canvas[0]), int(canvas[1])
        if (nh + ph, nw + pw) != (Hi, Wi):
            raise ValueError(f"the {whose}'s transforms lead to {(nh + ph, nw + pw)}, its image is {(Hi, Wi)}")
        N = int(input_ids.shape[0])
        if not isinstance(regions, (list, tuple)) or len(regions) != N:
            raise ValueError(f"regions: one list of region prompts per prompt ({N} prompts)")
        n_tok = (input_ids == REGION_TOKEN_INDEX).sum(1).tolist()
        prims, radii, masks, counts = [], [], [], []
        poly_rings, poly_verts, polys = [], [], []                # ring rows [region, first vertex, vertices, 0], vertices (x, y), the polygon regions

        def coord(v, what, where):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{where}: {what} {v!r} is not an integer pixel coordinate")
            return int(v)

        for b, entry in enumerate(regions):
            if not isinstance(entry, (list, tuple)) or len(entry) != n_tok[b]:
                got = len(entry) if isinstance(entry, (list, tuple)) else type(entry).__name__
                raise ValueError(f"prompt {b}: {got} region prompts for {n_tok[b]} <region> tokens")
            inst = seg_info[b].get("instances") if isinstance(seg_info[b], dict) else None
            if getattr(inst, "region_masks", None) is not None:
                raise ValueError(f"prompt {b}: regions given together with seg_info's instances.region_masks")
            counts.append(len(entry))
            for j, rp in enumerate(entry):
                where = f"prompt {b}, region {j}"
                g = len(radii)
                kinds = [k for k in self.REGION_PROMPT_KEYS if isinstance(rp, dict) and k in rp]
                if len(kinds) != 1:
                    raise ValueError(f"{where}: a region prompt is a dict with exactly one of {self.REGION_PROMPT_KEYS}, got "
                                     f"{sorted(rp) if isinstance(rp, dict) else type(rp).__name__}")
                kind = kinds[0]
                extra = sorted(set(rp) - {kind} - ({"radius"} if kind in self.REGION_PROMPT_RADIUS else set()))
                if extra:
                    raise ValueError(f"{where}: unknown keys {extra} in a {kind!r} prompt")
                if kind in self.REGION_PROMPT_RADIUS:
                    rad = rp.get("radius", self.REGION_PROMPT_RADIUS[kind])
                    if isinstance(rad, (bool, np.bool_)) or not isinstance(rad, (int, np.integer)) or not 0 <= int(rad) <= self.REGION_PROMPT_MAX_RADIUS:
                        raise ValueError(f"{where}: radius {rad!r} outside 0..{self.REGION_PROMPT_MAX_RADIUS}")
                    pix = list(rp[kind])
                    if not pix:
                        raise ValueError(f"{where}: an empty {kind!r} list")
                    for p in pix:
                        if len(p) != 2:
                            raise ValueError(f"{where}: {p!r} is not a (y, x) pair")
                        y, x = coord(p[0], "y", where), coord(p[1], "x", where)
                        if not (0 <= y < h and 0 <= x < w):
                            raise ValueError(f"{where}: pixel {(y, x)} outside the image of {(h, w)}")
                        prims.append((g, 0, y, x, 0, 0))
                    radii.append(int(rad))
                elif kind == "box":
                    if len(rp["box"]) != 4:
                        raise ValueError(f"{where}: a box is (y0, x0, y1, x1)")
                    y0, x0, y1, x1 = [coord(v, "box coordinate", where) for v in rp["box"]]
                    if not (0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w):
                        raise ValueError(f"{where}: box {(y0, x0, y1, x1)} is not 0 <= y0 < y1 <= {h}, 0 <= x0 < x1 <= {w}")
                    prims.append((g, 1, y0, x0, y1, x1))
                    radii.append(-1)
                elif kind == "polygon":
                    poly = rp["polygon"]
                    if not isinstance(poly, (list, tuple, np.ndarray)) or len(poly) == 0:
                        raise ValueError(f"{where}: a polygon is a ring [(y, x), ...] or a list of rings")
                    first = poly[0]
                    one_ring = isinstance(first, (list, tuple, np.ndarray)) and len(first) == 2 and not isinstance(first[0], (list, tuple, np.ndarray))
                    for ring in ([poly] if one_ring else poly):
                        if not isinstance(ring, (list, tuple, np.ndarray)) or len(ring) < 3:
                            n_v = len(ring) if isinstance(ring, (list, tuple, np.ndarray)) else 0
                            raise ValueError(f"{where}: a polygon ring of {n_v} vertices (at least 3)")
                        poly_rings.append((g, len(poly_verts), len(ring), 0))
                        for p in ring:
                            if not isinstance(p, (list, tuple, np.ndarray)) or len(p) != 2:
                                raise ValueError(f"{where}: {p!r} is not a (y, x) vertex")
                            y, x = coord(p[0], "y", where), coord(p[1], "x", where)
                            if not (0 <= y <= h and 0 <= x <= w):
                                raise ValueError(f"{where}: vertex {(y, x)} outside the lattice 0..{h} x 0..{w} of the image of {(h, w)}")
                            poly_verts.append((x, y))
                        if len(poly_verts) > self.REGION_POLYGON_MAX_VERTICES:
                            raise ValueError(f"{where}: the polygon prompts of one call hold more than {self.REGION_POLYGON_MAX_VERTICES} vertices")
                    polys.append(g)
                    radii.append(-1)
                else:
                    m = rle_to_mask(rp["rle"]) if kind == "rle" else rp["mask"]
                    if not torch.is_tensor(m):
                        m = np.asarray(m)
                    if tuple(m.shape) != (h, w):
                        raise ValueError(f"{where}: a mask of shape {tuple(m.shape)} for an image of {(h, w)}")
                    if m.dtype not in (torch.uint8, torch.bool, np.dtype(np.uint8), np.dtype(np.bool_)):
                        raise ValueError(f"{where}: a mask of dtype {m.dtype} (uint8 or bool)")
                    if torch.is_tensor(m) and m.device.type == "cpu":
                        m = m.numpy()
                    masks.append((g, m if torch.is_tensor(m) else np.ascontiguousarray(m != 0).view(np.uint8)))
                    radii.append(-1)
        R = len(radii)
        if R == 0:
            raise ValueError("regions given, but no prompt holds a <region> token")
        arrays = {f"region_img{tag}": np.zeros(R, np.int32),                                   # every region pools from the session's image
                  f"region_prims{tag}": np.asarray(prims, np.int32).reshape(-1, 6), f"region_radii{tag}": np.asarray(radii, np.int32)}
        for g, m in masks:
            if not torch.is_tensor(m):
                arrays[f"region_mask{tag}_{g}"] = m.reshape(-1)
        if polys:
            arrays[f"region_poly_rings{tag}"] = np.asarray(poly_rings, np.int32).reshape(-1)
            arrays[f"region_poly_verts{tag}"] = np.asarray(poly_verts, np.int32).reshape(-1)
        return {"tag": tag, "R": R, "counts": counts, "hw": (h, w), "tables": (h, w, nh, nw, ph, pw), "masks": masks, "arrays": arrays,
                "max_radius": max([0] + radii), "polygons": polys}

    def _region_prompt_masks(self, session, rp, dv, total, tables=None):
        """Device side, in front of the read-back: one launch each of rasterize, dilate and resize + pad for the R regions of `rp`; `total` (R) int32
        zeroed, receives the pixel totals of the resized masks.  Returns (masks (R, S, S) uint8, row_cnt (R, S)).  Without a session: `tables`,
        the (row, column) index tables of `rp["tables"]` on the device."""
        o = self.ops
        tag, R, (h, w) = rp["tag"], rp["R"], rp["hw"]
        tabs = (rp["tables"],) + tuple(tables) if session is None else session.region_tables
        if tabs is None or tabs[0] != rp["tables"]:
            from .preprocess import nearest_pad_tables
            rows, cols = nearest_pad_tables(*rp["tables"])
            tabs = session.region_tables = (rp["tables"], self._dev_i32(rows), self._dev_i32(cols))
        raw = o.mask_rasterize(dv[f"region_prims{tag}"].view(-1, 6), R, h, w)
        for g, m in rp["masks"]:                                  # mask prompts: into their (zeroed) plane as they are
            if torch.is_tensor(m):
                m = m.to(self.device).contiguous()
                src = m.view(torch.uint8) if m.dtype == torch.bool else m
            else:
                src = dv[f"region_mask{tag}_{g}"]
            o.copy_(raw[g], src.view(h, w))
        for g in rp["polygons"]:                                  # polygon prompts: filled even-odd into their plane (psalm_mask_fill_polygons)
            o.mask_fill_polygons(dv[f"region_poly_rings{tag}"].view(-1, 4), dv[f"region_poly_verts{tag}"].view(-1, 2), (R, h, w), rows=(g, 1),
                                 out=raw[g:g + 1])
        dil = o.mask_dilate_disc(raw, dv[f"region_radii{tag}"], rp["max_radius"])
        return o.mask_resize_nearest_pad(dil, tabs[1], tabs[2], total=total)

    def _region_prompt_ranks(self, rp, totals, sampler):
        """Behind the read-back: `sampler(m, n)` per region in order (prompt by prompt, region by region) -> (R, n) int32 ranks into each region's
        non-zero pixels.  A region without a pixel is an error here (the reference would fail in randint(0, 0))."""
        n = self.cfg.region_points
        out, g = [], 0
        for b, k in enumerate(rp["counts"]):
            for j in range(k):
                m = int(totals[g])
                if m <= 0:
                    raise ValueError(f"prompt {b}, region {j}: no pixel of the prompt is left after the resize to the model's input size")
                idx = torch.as_tensor(sampler(m, n)).reshape(-1).to(torch.int32)
                if idx.numel() != n:
                    raise ValueError(f"prompt {b}, region {j}: the region_index_sampler returned {idx.numel()} ranks, {n} are needed")
                out.append(idx)
                g += 1
        return torch.stack(out) if out else torch.zeros(0, n, dtype=torch.int32)

    def _region_pick(self, res):
        """`pick=True`: per region the best query (first arg-max of `instances.scores`' column), its score and its binary mask as bytes, from a
        post-processed region result that `_finalize` has not sliced yet."""
        o = self.ops
        _, scores, inst_masks, _ = res["_pending"]
        q, s = o.region_best(scores if scores.is_contiguous() else scores.contiguous())
        out = {"picked_query": o.to_i64(q), "picked_scores": s, "picked_masks": o.mask_gather_u8(inst_masks, q)}
        if self.mask_boxes:                      # the picked queries' planes through the index list: no gather copy
            out["picked_boxes"], out["picked_areas"] = o.mask_boxes(inst_masks, index=q)
        return out

    @torch.no_grad()
    def segment(self, session: "ImageSession", input_ids, attention_mask=None, *, seg_info=None, class_name_ids=None,
                class_name_embedding_indices=None, cls_indices=None, token_refer_id=None, refer_embedding_indices=None, is_thing_list=None,
                labels=None, region_point_sampler: Callable = default_region_point_sampler, postprocess: bool = True,
                stages: Optional[dict] = None, regions=None, region_index_sampler: Callable = default_region_index_sampler, pick: bool = True,
                outlines: bool = False, centers: bool = False):
        """N >= 1 prompts of the model's task on the session's image: what `eval_seg` returns for a batch of N copies of that image with these
        prompts (a list of N result dicts), without running the vision side again and with a Phi pass over the rows behind the shared prefix
        only.  Prompt-side keywords as eval_seg; `seg_info`: per prompt (region masks / ground truth under "instances", geometry), default the
        session's entry for every prompt.  All prompts must agree on the tokens up to and including their one <image> (ValueError otherwise).
        postprocess=False: the predictor outputs per prompt, as `forward_logits`; `stages`: filled as by `forward_logits(stages=...)` with the
        suffix rows' `inputs_embeds` / `hidden_states`.

        `regions` (region task): the region prompts as GEOMETRY instead of `instances.region_masks` -- per prompt a list with one dict per <region>
        token, in pixels of the ORIGINAL image (the (h, w) of the session's `seg_info["transforms"]["resize"]`):
            {"points": [(y, x), ...]}      discs of radius 10 ("radius": k overrides it, 0..16)
            {"scribble": [(y, x), ...]}    the stroke's pixels, radius 5 (same override)
            {"box": (y0, x0, y1, x1)}      half-open, 0 <= y0 < y1 <= h, 0 <= x0 < x1 <= w; not dilated
            {"mask": (h, w) uint8 / bool array or tensor, host or device}   used as it is (non-zero = set)
            {"rle": COCO RLE dict}         decoded on the host (preprocess.rle_to_mask), then a mask
            {"polygon": [(y, x), ...]}     a ring of >= 3 integer LATTICE vertices, 0 <= y <= h, 0 <= x <= w (pixel (py, px) covers [py, py + 1] x
                                           [px, px + 1]), or a list of such rings (holes are rings); filled even-odd over the pixel centres on the
                                           device (psalm_mask_fill_polygons: the rule of evalout.fill_polygons); not dilated
        The prompt is drawn, dilated, resized + padded and sampled on the device (psalm_mask_rasterize, psalm_mask_dilate_disc,
        psalm_mask_resize_nearest_pad, psalm_mask_select_points: one launch each per call, one read-back of the R pixel totals);
        `region_index_sampler(m, n)` draws n ranks into the m pixels of a region, prompt by prompt, region by region.  The results equal, bit for
        bit, those of the host path on `apply_segmentation(enhance_with_circles(mask, radius), transforms)` as `region_masks` under
        `region_point_sampler = lambda nz, k: region_index_sampler(nz.shape[0], k)`.  With `regions`, `gt` is returned only where the prompt's
        seg_info carries `instances.gt_masks`, and `pick=True` adds `picked_query` (R) int64, `picked_scores` (R) float32, `picked_masks`
        (R, H, W) uint8 (device tensors): per region the first arg-max of `instances.scores` and that query's mask -- and, with the model's
        `mask_boxes` switch on, `picked_boxes` (R, 4) float32 / `picked_areas` (R) int32 of those masks.  `outlines=True` (with `pick`) adds
        `picked_outlines`: evalout.mask_outlines of `picked_masks` (connectivity 8), the polygons of those masks as device tables.
        `centers=True` (with `pick`) adds `picked_centers` (R, 3) int32 on the device: evalout.mask_centers of `picked_masks`, per region
        [y, x, dist2] of the mask's pixel deepest inside ([-1, -1, 0]: an empty mask) -- (y, x) is a {"points": [(y, x)]} prompt of the next call.
        It is computed behind everything else; anything but a bool raises ValueError."""
        kw = dict(input_ids=input_ids, attention_mask=attention_mask, seg_info=seg_info, class_name_ids=class_name_ids,
                  class_name_embedding_indices=class_name_embedding_indices, cls_indices=cls_indices, token_refer_id=token_refer_id,
                  refer_embedding_indices=refer_embedding_indices, is_thing_list=is_thing_list, regions=regions)
        return self._segment_requests([(session, kw)], grouped=False, postprocess=postprocess, stages=stages,
                                      region_point_sampler=region_point_sampler, region_index_sampler=region_index_sampler, pick=pick,
                                      outlines=outlines, centers=centers)[0]

    @torch.no_grad()
    def segment_many(self, requests, *, postprocess: bool = True, region_point_sampler: Callable = default_region_point_sampler,
                     stages: Optional[dict] = None, region_index_sampler: Callable = default_region_index_sampler, pick: bool = True,
                     outlines: bool = False, centers: bool = False):
        """Prompts on SEVERAL images in one Phi pass: `requests` is a list of (session, kwargs) pairs, kwargs what `segment(session, **kwargs)` takes
        for the prompt side (input_ids, attention_mask, seg_info, class_name_ids, ..., is_thing_list).  Returns one list per request, each what
        `segment(session, **kwargs)` returns.  Every request obeys segment's rules on its own (session of this model and weights version, its
        prompts agree up to and including <image>); requests may differ in image size, n_img, leading text and so in prefix length.  A session may
        appear in several requests -- they share its one prefix cache, so they must share their leading text too.
        The prefix caches are built or reused per session as `segment` does it; then ONE suffix pass runs over the prompts of all requests (S = the
        bucketed maximum of their suffix lengths) with the grouped prefix attention, the row-set means and projector GEMMs run once, and the
        predictor and post-processing run per prompt from its own session.
        Region task: `region_point_sampler` is called request by request in list order, inside a request prompt by prompt and region by region --
        the order a loop of `segment` calls over `requests` draws in.
        A request's kwargs may carry `regions` (and `pick`, `outlines`, `centers`) as `segment` takes them: the prompt masks are made per request on the device, ONE read-back
        brings the pixel totals of all requests, and `region_index_sampler` is called request by request, prompt by prompt, region by region.  Either
        every region request of a call gives `regions` or none does (the two paths draw from the sampler at different points of the call).
        `stages`: filled with the suffix rows' `inputs_embeds` / `hidden_states` ((N, S, hidden), N = all prompts in request order), `prefix_lens`
        (per prompt) and `lengths`."""
        return self._segment_requests(list(requests), grouped=True, postprocess=postprocess, stages=stages, region_point_sampler=region_point_sampler,
                                      region_index_sampler=region_index_sampler, pick=pick, outlines=outlines, centers=centers)

    def _segment_requests(self, requests, *, grouped: bool, postprocess, stages, region_point_sampler, region_index_sampler, pick, outlines=False,
                          centers=False):
        """The one pipeline behind `segment` (grouped = False: its one request) and `segment_many` (grouped = True): a list of (session, kwargs)
        pairs -> one list of results per request.  Per request: validation, the region prompts' host side, the suffix splice plan; then the
        prefix caches (one per session), ONE blob with the suffix plans side by side, the region masks / points / features, ONE Phi suffix pass,
        the decoder embeddings, the mask decoder per session and the post-processing per prompt.
        `grouped` chooses how the suffix rows attend the prefix -- False: the request's own cache (psalm_phi_suffix), True: the table of cache
        references in the blob (psalm_phi_suffix_grouped), also for a single request --, which keys `stages` receives, and the head of the error
        texts ("segment: " / "segment_many: request r: ")."""
        self._session_mode_check()
        if not requests:
            raise ValueError("segment_many: an empty request list")
        o, w, cfg = self.ops, self.w, self.cfg
        at = (lambda r: f"segment_many: request {r}: ") if grouped else (lambda r: "segment: ")
        for r, (_, kw) in enumerate(requests):
            if isinstance(kw, dict) and not isinstance(kw.get("centers", centers), (bool, np.bool_)):
                raise ValueError(f"{at(r)}centers = {kw.get('centers', centers)!r} (True or False)")
        plans, arrays = [], {}
        any_regions = False
        rps = []                                                  # per request: the plan of its `regions`, or None
        for r, (session, kw) in enumerate(requests):
            if not isinstance(session, ImageSession) or session.model is not self:
                raise ValueError(f"{at(r)}this session was made by another model (or replica)")
            if session.version != self._weights_version:
                raise ValueError(f"{at(r)}the model's weights were prepared again after this session was made; encode the image again")
            kw = dict(kw)
            if self.seg_task == "panoptic" and postprocess:
                assert kw.get("is_thing_list") is not None, "is_thing_list need to be given"
                self.is_thing_list = kw["is_thing_list"]
            ids = kw["input_ids"]
            if ids.dim() == 1:
                ids = ids[None]
            N = int(ids.shape[0])
            seg_info = kw.get("seg_info")
            if seg_info is None:
                seg_info = [session.seg_info if session.seg_info is not None else {}] * N
            if len(seg_info) != N:
                raise ValueError(f"{at(r)}one seg_info entry per prompt")
            n_regions = None
            rps.append(None)
            if kw.get("regions") is not None:
                try:
                    rps[r] = self._region_prompt_plan(session, ids, seg_info, kw["regions"], tag=str(r))
                except ValueError as e:
                    raise ValueError(f"{at(r)}{e}") from None
                n_regions = rps[r]["counts"]
                arrays.update(rps[r]["arrays"])
                any_regions = True
            elif bool((ids == REGION_TOKEN_INDEX).any()):
                pts, n_regions = self.region_points([s_["instances"].region_masks.tensor for s_ in seg_info], region_point_sampler)
                arrays[f"region_img{r}"] = np.zeros(sum(n_regions), np.int32)         # every region pools from its own session's image
                arrays[f"region_pts{r}"] = np.ascontiguousarray(pts.numpy(), np.float32)
                any_regions = True
            try:
                sp = self._session_plan(session, ids, kw.get("attention_mask"), kw.get("class_name_ids"), kw.get("cls_indices"),
                                        kw.get("token_refer_id"), n_regions, kw.get("class_name_embedding_indices") is not None,
                                        kw.get("refer_embedding_indices") is not None)
            except ValueError as e:
                if not grouped:                                   # (_session_plan's texts are segment's own: "segment: prompt ...")
                    raise
                raise ValueError(f"{at(r)}{e}") from None
            plans.append((session, sp, N, seg_info, n_regions))
        if any(p is not None for p in rps) and any(p is None and pl[4] is not None for p, pl in zip(rps, plans)):
            raise ValueError("segment_many: some requests give `regions`, others instances.region_masks: one kind per call")
        for name in ("cls", "refer", "region"):
            if len({sp[name] is None for _, sp, _, _, _ in plans}) != 1:
                raise ValueError(f"segment_many: some requests carry {name} rows and some do not; all requests are prompts of the model's one task")
        # the prefix caches, built or reused per session (a session listed twice: once)
        caches, cache_of, seen = [], [], {}
        for r, (session, sp, N, _, _) in enumerate(plans):
            if id(session) in seen:
                c, first = seen[id(session)]
                if plans[first][1]["key"] != sp["key"] or plans[first][1]["P"] != sp["P"]:
                    raise ValueError(f"segment_many: requests {first} and {r} share a session but not their leading text (one prefix cache per session)")
            else:
                c = len(caches)
                caches.append(self._session_prefix(session, sp))
                seen[id(session)] = (c, r)
            cache_of += [c] * N
        Nt = len(cache_of)
        S = max(sp["S"] for _, sp, _, _, _ in plans)
        P_max = max(sp["P"] for _, sp, _, _, _ in plans)
        # the suffix plans side by side: prompt g of the call = prompt b of its request; rows re-based from (b, s) of (N_r, S_r) to (g, s) of (Nt, S)
        sid = np.full((Nt, S), -1, np.int32)
        srow = np.zeros((Nt, S), np.int32)
        kmask = np.zeros((Nt, S), np.uint8)
        sets = {name: ([np.zeros(1, np.int32)], []) for name in ("seg", "cls", "refer", "region") if plans[0][1][name] is not None}
        g0 = reg0 = 0
        for session, sp, N, _, n_regions in plans:
            Sr = sp["S"]
            sid[g0:g0 + N, :Sr], kmask[g0:g0 + N, :Sr] = sp["sid"], sp["kmask"]
            assert not (sp["sid"] == 1).any(), "image rows live in the prefix"
            srow[g0:g0 + N, :Sr] = sp["srow"] + np.where(sp["sid"] == 3, reg0, 0).astype(np.int32)      # region rows: into the concatenated features
            for name, (offs, rows) in sets.items():
                off, rw = sp[name]
                n = int(off[-1])
                rw = rw[:n].astype(np.int64)                     # (behind off[-1]: _session_plan's bucket padding)
                rows.append(((rw // Sr + g0) * S + rw % Sr).astype(np.int32))
                offs.append((off[1:].astype(np.int64) + int(offs[-1][-1])).astype(np.int32))
            g0 += N
            reg0 += sum(n_regions) if n_regions else 0
        q = max(int(self.len_bucket or 0), 1)
        for name, (offs, rows) in sets.items():
            rows = np.concatenate(rows) if rows else np.zeros(0, np.int32)
            if name != "seg" and q > 1:                           # (as _session_plan buckets the row-set lengths)
                n = (rows.shape[0] + q - 1) // q * q
                rows = np.concatenate((rows, np.zeros(max(n, q) - rows.shape[0], np.int32)))
            arrays[name + "_off"], arrays[name + "_rows"] = np.concatenate(offs), rows
        arrays["sid"], arrays["srow"], arrays["kmask"] = sid.reshape(-1), srow.reshape(-1), kmask.reshape(-1)
        rhost = None
        if grouped:                                               # (the table holds cache pointers: the caches exist before the blob is packed)
            rhost = o.prefix_ref_table(caches, cache_of)
            arrays["refs"] = rhost.view(np.uint8).reshape(-1)
        blob, layout = self._pack(arrays)
        dv = self._views(torch.from_numpy(blob).to(self.device), layout)
        region_feats = None
        dev_pts = {}
        if any(p is not None for p in rps):                      # `regions`: masks per request, ONE read-back of all totals, then the sampler in request order
            total = o.zeros(sum(p["R"] for p in rps if p is not None), dtype=torch.int32)
            made, g0 = {}, 0
            for r, p in enumerate(rps):
                if p is not None:
                    made[r] = self._region_prompt_masks(plans[r][0], p, dv, total[g0:g0 + p["R"]])
                    g0 += p["R"]
            totals = total.cpu().tolist()
            ranks, g0 = {}, 0
            for r, p in enumerate(rps):
                if p is not None:
                    try:
                        ranks[r] = self._region_prompt_ranks(p, totals[g0:g0 + p["R"]], region_index_sampler)
                    except ValueError as e:
                        raise ValueError(f"{at(r)}{e}") from None
                    g0 += p["R"]
            idx = torch.cat([ranks[r] for r in sorted(ranks)]).to(self.device)
            g0 = 0
            for r in sorted(ranks):
                dev_pts[r] = o.mask_select_points(made[r][0], made[r][1], idx[g0:g0 + rps[r]["R"]])
                g0 += rps[r]["R"]
        if any_regions:
            feats = []
            for r, (session, sp, N, _, n_regions) in enumerate(plans):
                if n_regions is None:
                    continue
                side = int(math.sqrt(session.n_img))
                pts = dev_pts[r] if r in dev_pts else dv[f"region_pts{r}"].view(sum(n_regions), -1, 2)
                feats.append(o.region_pool(session.image_tokens, dv[f"region_img{r}"], pts, side, side, session.n_img))
            region_feats = feats[0] if len(feats) == 1 else torch.cat(feats)
        embeds = o.gather_rows([w["embed"], None, w["seg_query"], region_feats], dv["sid"], dv["srow"], cfg.hidden_size, out_dtype=torch.float32)
        hidden = self._llm_session(embeds, dv["kmask"].view(Nt, S), Nt, S, P_max, None if grouped else caches[0], suffix=True,
                                   refs=(dv["refs"], rhost) if grouped else None)
        seg_q, cls_emb, seg_emb, reg_emb = self._decoder_embeddings(hidden, dv)
        if stages is not None and grouped:
            stages.update(prefix_lens=[sp["P"] for _, sp, N, _, _ in plans for _ in range(N)],
                          lengths=[l_ for _, sp, _, _, _ in plans for l_ in sp["lens"]],
                          inputs_embeds=embeds.view(Nt, S, -1), hidden_states=hidden.view(Nt, S, -1))
        elif stages is not None:
            session, sp = plans[0][:2]
            Sr = sp["S_real"]
            stages.update(feats=session.feats, image_tokens=session.image_tokens, prefix_len=P_max, lengths=sp["lens"],
                          inputs_embeds=embeds.view(Nt, S, -1)[:, :Sr], hidden_states=hidden.view(Nt, S, -1)[:, :Sr],
                          seg_query=seg_q.view(Nt, cfg.md_queries, -1), class_name_embedding=cls_emb, SEG_embedding=seg_emb, region_embedding=reg_emb,
                          mask_features=[session.mask_features] * Nt, multi_scale_features=[session.multi_scale_features] * Nt)
        # every prompt's decoder operands, then the prompts of all requests naming one session as one batch of the decoder (different sessions have
        # different K / V: separate calls)
        prompts = list(self._prompt_operands(seg_q, cls_emb, seg_emb, reg_emb, [nc for _, sp, _, _, _ in plans for nc in sp["n_cls"]],
                                             [k for pl in plans for k in (pl[4] or ())]))
        by_session, g = {}, 0
        for session, _, N, _, _ in plans:
            by_session.setdefault(id(session), (session, []))[1].extend(range(g, g + N))
            g += N
        decoded = {}
        for session, gs in by_session.values():
            rs = self._decode_batched(session, [prompts[i] for i in gs])
            if rs is not None:
                decoded.update(zip(gs, rs))
        results = []
        g = 0
        for ri, (session, sp, N, seg_info, n_regions) in enumerate(plans):
            mf, ms, shapes, mfs = session.mask_features, session.multi_scale_features, session.shapes, session.mask_features_size
            Hi, Wi = int(session.images.shape[2]), int(session.images.shape[3])
            outs = []
            for b in range(N):
                sq, se, ce, re = prompts[g]
                res = decoded[g] if g in decoded else self.predictor(ms, shapes, mf, mfs, sq, se, ce, re,
                                                                     kv=self._session_kv(session, n_regions[b] if n_regions else 0))
                g += 1
                if postprocess:
                    res = self._postprocess(res, self._post_sizes(Hi, Wi, seg_info[b], cfg.size_divisibility))
                    picked = self._region_pick(res) if rps[ri] is not None and requests[ri][1].get("pick", pick) and n_regions[b] else {}
                    res = self._finalize(res, seg_info[b], gt_optional=rps[ri] is not None)
                    if picked and requests[ri][1].get("outlines", outlines):
                        from .evalout import mask_outlines
                        picked["picked_outlines"] = mask_outlines(picked["picked_masks"], connectivity=8, ops=o)
                    if picked and requests[ri][1].get("centers", centers):
                        from .evalout import mask_centers
                        picked["picked_centers"] = mask_centers(picked["picked_masks"], ops=o)
                    res.update(picked)
                outs.append(res)
            results.append(outs)
        return results

    @torch.no_grad()
    def segment_everything(self, session: "ImageSession", input_ids, attention_mask=None, *, grid=(8, 8), regions=None, radius=None,
                           iou_thr=0.7, min_area: int = 1, min_score: Optional[float] = None,
                           region_index_sampler: Callable = default_region_index_sampler, min_island: int = 0, max_hole: int = 0,
                           connectivity: int = 8, outlines: bool = False, centers: bool = False):
        """"Show me all the objects": a grid of clicks on the session's image, one mask per object back.  `input_ids` (N, T): region-task prompts
        on the session's image that hold R <region> tokens together, 1 <= R <= 1024.  Either `grid=(gy, gx)` with gy * gx == R -- one click per
        cell at the cell centre ((2 i + 1) h // (2 gy), (2 j + 1) w // (2 gx)) of the original (h, w), dealt to the prompts in row-major order by
        their token counts, `radius` overriding the click's radius -- or `regions` in the grammar of `segment(regions=)` (then pass grid=None).

        One call of the pipeline behind `segment(..., regions=..., pick=True)`; then, all on the device: the picked queries' planes of every
        prompt are packed into ONE (R, nw) bit buffer through the index list (psalm_mask_pack_bits: no byte gather), all-pairs intersections
        (psalm_mask_pair_counts), greedy NMS (psalm_mask_nms: descending picked score, equal scores the lower click first; a mask of fewer than
        `min_area` pixels or a score below `min_score` is filtered; a click whose mask's IoU with an already kept one EXCEEDS `iou_thr` --
        compared as the rational of evalout.iou_fraction, 0.7 = 7/10, strictly -- is suppressed by the first such one) and the label map
        (psalm_mask_paint_bits).  ONE read-back, the kept block; then the K survivors are unpacked (psalm_mask_unpack_bits) and boxed
        (psalm_mask_boxes, whatever the `mask_boxes` switch says).

        Returns device tensors, survivors by descending score: `masks` (K, H, W) uint8, `scores` (K) float32, `queries` (K) int64, `regions` (K)
        int64 (the click behind each survivor, flat over the prompts), `areas` (K) int32, `boxes` (K, 4) float32 (the `mask_boxes` convention),
        `labels` (H, W) int32 (0: background, k + 1: survivor k; the better score wins a contested pixel), `owner` (R) int64 (per click the click
        whose mask stands for it, -1: filtered), `keep` (R) int32 (1 kept, 0 suppressed, -1 filtered), `prompts` (what `segment` returned).

        `min_island` / `max_hole` > 0 clean every click's picked mask first (psalm_mask_clean: holes of at most max_hole pixels, judged under the
        complementary connectivity, are filled; then islands of fewer than min_island pixels under `connectivity` are dropped) and everything
        above -- pair counts, NMS with `min_area` on the cleaned area, the label map, `masks`, `areas`, `boxes` -- describes the cleaned masks;
        the result gains `cleaned` (R, 2) int32 = [removed, filled] pixels per click.  With both 0 the call is launch for launch the one
        without them.

        `outlines=True`: the result gains `outlines`, evalout.mask_outlines of the K returned `masks` under the call's `connectivity` -- the
        survivors as polygons (`evalout.outline_polygons` lists them; COCO `segmentation` lists as they stand) -- behind everything else: every
        other key and every launch in front of it are those of the call without it.

        `centers=True`: the result gains `centers` (K, 3) int32, evalout.mask_centers of the K returned `masks`: per survivor [y, x, dist2] of the
        pixel deepest inside it, the image border counted as outside -- a click in the original image's pixels, the space of `regions=`:
        {"points": [(y, x)]} re-prompts `segment` or starts a `VideoTracker` on that object.  Computed behind everything else (behind
        `outlines`), with the same guarantee; anything but a bool raises ValueError."""
        from .evalout import iou_fraction
        if self.seg_task != "region":
            raise ValueError(f"segment_everything: clicks are prompts of the region task (this model's seg_task = {self.seg_task!r})")
        if not isinstance(session, ImageSession) or session.model is not self:
            raise ValueError("segment_everything: this session was made by another model (or replica)")
        try:
            num, den = iou_fraction(iou_thr)
        except ValueError as e:
            raise ValueError(f"segment_everything: {e}") from None
        for name, v in (("min_island", min_island), ("max_hole", max_hole)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError(f"segment_everything: {name} = {v!r} (an integer >= 0)")
        if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
            raise ValueError(f"segment_everything: connectivity = {connectivity!r} (4 or 8)")
        if not isinstance(centers, (bool, np.bool_)):
            raise ValueError(f"segment_everything: centers = {centers!r} (True or False)")
        ids = input_ids[None] if input_ids.dim() == 1 else input_ids
        n_tok = (ids == REGION_TOKEN_INDEX).sum(1).tolist()
        R = int(sum(n_tok))
        if not 1 <= R <= 1024:
            raise ValueError(f"segment_everything: the prompts hold {R} <region> tokens (1..1024)")
        if (grid is None) == (regions is None):
            raise ValueError("segment_everything: give either `grid` or `regions` (with `regions`, pass grid=None)")
        if grid is not None:
            ok = isinstance(grid, (tuple, list)) and len(grid) == 2 and all(
                isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and v >= 1 for v in grid)
            if not ok or int(grid[0]) * int(grid[1]) != R:
                raise ValueError(f"segment_everything: grid {grid!r} for {R} <region> tokens (gy * gx must equal their number)")
            tr = session.seg_info.get("transforms") if isinstance(session.seg_info, dict) else None
            if tr is None:
                raise ValueError("segment_everything: regions need the session's seg_info['transforms'] (the resize / pad record of the image: "
                                 "encode_image(images, seg_info))")
            h, w = int(tr["resize"][0]), int(tr["resize"][1])
            gy, gx = int(grid[0]), int(grid[1])
            extra = {} if radius is None else {"radius": radius}
            clicks = [dict(points=[((2 * i + 1) * h // (2 * gy), (2 * j + 1) * w // (2 * gx))], **extra) for i in range(gy) for j in range(gx)]
            regions, g0 = [], 0
            for k in n_tok:
                regions.append(clicks[g0:g0 + k])
                g0 += k
        elif radius is not None:
            raise ValueError("segment_everything: `radius` overrides the radius of the grid's clicks; with `regions`, give it per region prompt")
        kw = dict(input_ids=input_ids, attention_mask=attention_mask, regions=regions)
        prompts = self._segment_requests([(session, kw)], grouped=False, postprocess=True, stages=None,
                                         region_point_sampler=default_region_point_sampler, region_index_sampler=region_index_sampler, pick=True)[0]
        out = self._everything_dedup(prompts, n_tok, num, den, min_area, min_score, int(min_island), int(max_hole), int(connectivity),
                                     outlines=bool(outlines), centers=bool(centers))
        out["prompts"] = prompts
        return out

    def _everything_dedup(self, prompts, n_tok, num, den, min_area, min_score, min_island=0, max_hole=0, connectivity=8, outlines=False,
                          centers=False):
        """The device step behind the pipeline: `prompts`, what `segment(..., pick=True)` returned for prompts of n_tok[b] regions each ->
        segment_everything's result without "prompts".  Reads `instances.pred_masks`, `picked_query` and `picked_scores` of every prompt.
        min_island / max_hole > 0: the picked planes are cleaned (psalm_mask_clean) into one (R, H, W) byte buffer, which is packed instead.
        outlines: behind everything else, the K survivors' masks as polygons (evalout.mask_outlines under `connectivity`).
        centers: behind that, the K survivors' deepest pixels (evalout.mask_centers)."""
        o = self.ops
        R = int(sum(n_tok))
        sizes = {tuple(p["instances"].pred_masks.shape[1:]) for p in prompts}
        if len(sizes) != 1:
            raise ValueError(f"segment_everything: the prompts produced masks of different sizes {sorted(sizes)}")
        Hh, Ww = sizes.pop()
        bits = o.empty(R, o.mask_bits_words(Hh * Ww), dtype=torch.int64)
        areas = o.empty(R, dtype=torch.int32)
        clean = min_island > 0 or max_hole > 0
        if clean:
            cleaned_planes = o.empty(R, Hh, Ww, dtype=torch.uint8)
            cleaned = o.empty(2, R, dtype=torch.int32)             # rows: removed, filled
        g0 = 0
        for k, p in zip(n_tok, prompts):                          # the picked queries' planes, prompt by prompt, into rows g0 .. g0 + k of the one buffer
            if k:
                planes = p["instances"].pred_masks
                planes = planes if planes.is_contiguous() else planes.contiguous()
                if clean:
                    o.mask_clean(planes, index=p["picked_query"].to(torch.int32), connectivity=connectivity, min_island=min_island, max_hole=max_hole,
                                 out=cleaned_planes[g0:g0 + k], out_areas=areas[g0:g0 + k], out_filled=cleaned[1, g0:g0 + k],
                                 out_removed=cleaned[0, g0:g0 + k])
                else:
                    o.mask_pack_bits(planes, index=p["picked_query"].to(torch.int32), out_bits=bits[g0:g0 + k], out_areas=areas[g0:g0 + k])
                g0 += k
        if clean:
            o.mask_pack_bits(cleaned_planes, out_bits=bits, want_areas=False)      # the areas are those of the cleaned planes already
        with_regions = [p for k, p in zip(n_tok, prompts) if k]
        scores = with_regions[0]["picked_scores"] if len(with_regions) == 1 else torch.cat([p["picked_scores"] for p in with_regions])
        queries = with_regions[0]["picked_query"] if len(with_regions) == 1 else torch.cat([p["picked_query"] for p in with_regions])
        inter = o.mask_pair_counts(bits)
        kept, keep, owner = o.mask_nms(inter, areas, scores.contiguous(), num, den, min_area=min_area, min_score=min_score)
        labels = o.mask_paint_bits(bits, kept, (Hh, Ww))
        K = int(kept.cpu()[0])                                    # the one read-back
        if K:
            rows = kept[1:1 + K]
            masks = o.mask_unpack_bits(bits, (Hh, Ww), rows=rows)
            boxes, kept_areas = o.mask_boxes(masks)
            which = o.to_i64(rows)
        else:
            masks = o.empty(0, Hh, Ww, dtype=torch.uint8)
            boxes, kept_areas, which = o.empty(0, 4), o.empty(0, dtype=torch.int32), o.empty(0, dtype=torch.int64)
        out = {"masks": masks, "scores": scores[which], "queries": queries[which], "regions": which, "areas": kept_areas, "boxes": boxes,
               "labels": labels, "owner": o.to_i64(owner), "keep": keep}
        if clean:
            out["cleaned"] = cleaned.t().contiguous()
        if outlines:
            from .evalout import mask_outlines
            out["outlines"] = mask_outlines(masks, connectivity=connectivity, ops=o)
        if centers:
            from .evalout import mask_centers
            out["centers"] = mask_centers(masks, ops=o)
        return out
