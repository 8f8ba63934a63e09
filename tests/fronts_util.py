"""Helper of the session-front tests (tests/test_31_session_fronts_emu.py, tests/test_32_session_fronts_gpu.py): `PSALM.segment(s, **kw)` and
`PSALM.segment_many([(s, kw)])` are two fronts of one pipeline (`_segment_requests`, psalm_amd/session.py), so for the same request they issue the
same launches in the same order and return the same bits.  Inputs and models are those of interactive_util (tiny models, 96 x 96 images)."""
from interactive_util import as_point_sampler, host_infos, image_of, model_for, prompts_of, rank_sampler, regions_for
from psalm_amd.synthetic import fix_indices, session_inputs
from session_util import seg_kwargs
from test_17_segment_many_emu import _same


def _front_calls(calls):
    """`segment`'s launch names as `segment_many` issues them for the same request -- the two permitted differences: the suffix entry's name, and
    psalm_phi_suffix's query of the cache size in front of it"""
    i = calls.index("psalm_phi_suffix")
    assert calls.count("psalm_phi_suffix") == 1 and calls[i - 1] == "psalm_phi_prefix_cache_bytes" and "psalm_phi_suffix_grouped" not in calls
    return calls[:i - 1] + ["psalm_phi_suffix_grouped"] + calls[i + 1:]


def fronts_case(kind, what):
    """kind: "emu" | "hip".  what: "referring" (3 sentences), "host_masks" / "regions" (region task, prompts of 1 and 3 regions as
    instances.region_masks / as geometry).  The launch names of the two fronts agree up to `_front_calls`, cold (the prefix cache is built) and warm
    (it is reused), and the results are equal bit for bit.  f16x3: the mode whose suffix pass is one native entry."""
    model = model_for(kind, "f16x3", "referring" if what == "referring" else "region")
    cfg = model.cfg
    samplers = {}
    if what == "referring":
        inp = fix_indices(session_inputs(cfg, "referring", 3, size=96))
        img, info = inp["images"][:1], inp["seg_info"][0]
        kw = {k: v for k, v in seg_kwargs(inp).items() if k != "is_thing_list"}
    else:
        img, info = image_of(cfg)
        h, w = info["transforms"]["resize"][:2]
        ids, am = prompts_of(cfg)
        regions = regions_for(h, w)
        if what == "regions":
            kw, samplers = {"input_ids": ids, "attention_mask": am, "regions": regions}, {"region_index_sampler": rank_sampler}
        else:
            kw = {"input_ids": ids, "attention_mask": am, "seg_info": host_infos(info, regions)}
            samplers = {"region_point_sampler": as_point_sampler(rank_sampler)}
    lib = model.ops.lib
    runs = {}
    for front in ("segment", "segment_many"):
        sess = model.encode_image(img, info)                     # a fresh session per front: its first call is cold, its second warm
        for phase in ("cold", "warm"):
            lib.calls = []
            try:
                out = model.segment(sess, **kw, **samplers) if front == "segment" else model.segment_many([(sess, kw)], **samplers)[0]
                runs[front, phase] = (lib.calls, out)
            finally:
                lib.calls = None
        assert (sess.prefix_builds, sess.prefix_hits) == (1, 1)
    for phase in ("cold", "warm"):
        (one, got), (many, want) = runs["segment", phase], runs["segment_many", phase]
        assert many.count("psalm_phi_suffix_grouped") == 1 and "psalm_phi_suffix" not in many
        assert ("psalm_phi_prefix" in many) == (phase == "cold")
        assert _front_calls(one) == many, phase
        assert len(got) == int(kw["input_ids"].shape[0])
        _same(got, want, phase)
