"""KV-cached generation timing at full model size (random init, params.init_value): prefill of one image + ~1.5k text tokens, then ms per
generated token for B = 1 and B = 8 over --new tokens, with and without the captured step, and the host's enqueue time per step.  Prints
one JSON line (and writes it to --out).  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script
(--profile: fewer tokens, B = 1 and 8, graph on).

  python tools/decode_bench.py --model llama3 --out profiles/decode_bench_llama3.json
  python tools/decode_bench.py --model phi3 --out profiles/decode_bench_phi3.json

--weights fp8: the decoder (and lm_head) is quantised to FP8 weight-only form first (Engine.quantize_decoder, with write-back), then every
batch size runs the bf16 leg (the fp8 copies hidden: the bf16 kernels on the written-back weights) and the fp8 leg alternately, --repeats
times each, in this one process on the same engine and prompts; the JSON carries both legs, their medians, the spread (max - min) of the
bf16 leg and the ratio.  A gain counts only where the fp8 median is below the bf16 median by more than that spread.

  python tools/decode_bench.py --model llama3 --weights fp8 --out profiles/decode_bench_llama3_fp8.json

--weights mxfp4: one engine, quantised to MXFP4 with write-back (Engine.quantize_decoder(fmt="mxfp4")); e4m3 copies of the same written-back
weights are made beside them without a second write-back (only their time matters).  Three legs alternate, --repeats runs each, in one
process: the bf16 kernels on the written-back weights, the fp8 leg, the mxfp4 leg.  A cell is a "gain" only if the slowest mxfp4 run lies
below the fastest fp8 run.

  python tools/decode_bench.py --model llama3 --weights mxfp4 --out profiles/decode_bench_llama3_mxfp4.json

--kv fp8: the engine is quantised to --weights (bf16: left as it is) and stays in that format; the bf16-cache leg and the fp8-cache leg
(kv_cache_dtype="fp8_e4m3": e4m3fn bytes + one scale per (token, KV head)) alternate, --repeats runs each, in one process on the same
engine and prompts.  The JSON carries every run and the cache bytes of both legs.  A cell is a "gain" only if the slowest fp8-cache run lies
below the fastest bf16-cache run.

  python tools/decode_bench.py --model phi3 --weights mxfp4 --kv fp8 --out profiles/decode_bench_phi3_kvfp8.json

--lookup N: prompt-lookup decoding with N drafts per step at the chosen --weights / --kv (fp8: the fp8 cache).  Three legs alternate,
--repeats runs each, in one process on the same engine and prompts: the plain step (which also records the greedy continuation), the verify
step with a drafter that is always wrong (acceptance 0: the pure cost of a verify step) and with the recorded continuation (every draft
accepted).  Each leg reads its tokens on the host once per step, as generate() does.  Reported: ms per plain step, ms per verify step and
their ratio c; a verify step emits 1 + a tokens, so lookup pays when the mean number of accepted drafts per step a exceeds c - 1.  The
tool asserts that both lookup legs reproduce the plain leg's tokens.  Batch sizes with B (N + 1) > 16 are skipped.  Default --out:
profiles/decode_bench_{llama3,phi3}_lookup.json.

  python tools/decode_bench.py --model llama3 --lookup 7 --batches 1

--wide: 17 .. 64 sequences per step at the chosen --weights (the engine stays in that format).  Per batch size (default 16,32,64) the wide
leg (one vp_decode_gemm*_wide call per GEMM) and the chunked leg (DecodeSession.wide_gemm = False: the M <= 16 entry point once per 16-row
slice) alternate, --repeats runs each, in one process on the same engine and prompts; at B = 16 both legs are the M <= 16 kernel (the
yardstick of the run-to-run spread).  The prompt is --text tokens + one image; where a batch does not fit, the text is shortened by a
quarter until it does, and every run records the text_tokens it used.  A cell is a "gain" only if the slowest wide run lies below the
fastest chunked run.  Default --out: profiles/decode_bench_{llama3,phi3}_wide.json, which collects the cells of every --weights run.

  python tools/decode_bench.py --model llama3 --wide --weights mxfp4

--select: token selection between two steps, torch against the device selector (vp_decode_select).  Per batch size (default 1,8,64) and
for eager launches and the captured step, three legs alternate, --repeats runs each, in one process on the same engine and prompts:
  torch        what generate() does per token without the new arguments: step, decode.next_tokens(do_sample, temperature 0.8, top_p 0.9:
               sort, softmax, cumsum, scatter, multinomial), the EOS / pad bookkeeping and its host read of `finished` every token
  device       the same sampling configuration selected on the device at the end of the step, `finished` read every token (sync_every 1)
  device_k50   the device leg with top_k 50 and repetition_penalty 1.1 on top, `finished` read every 16 tokens (no torch counterpart)
Sampling with temperature 0.8, top_p 0.9 is the one sampled configuration both paths can run.  The EOS id is one that stops nothing, so
every leg decodes --new tokens.  A cell is a "gain" only if the slowest device run lies below the fastest torch run (and a "loss" the other
way round); device_k50 is reported beside them.  The logits are a random-init model's: nearly flat, so top_p 0.9 keeps most of the
vocabulary, which is the selector's most expensive case.  Where a batch does not fit, the text is shortened by a quarter until it does.
Default --out: profiles/decode_bench_{llama3,phi3}_select.json.

  python tools/decode_bench.py --model llama3 --select
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(model, layers):
    from visper_lm_amd.config import llama3_8b, phi3_mini
    from visper_lm_amd.engine import Engine
    kw = dict(aux_mode="", num_task_tokens=0)
    if layers:
        kw["num_hidden_layers"] = layers
    cfg = llama3_8b(**kw) if model == "llama3" else phi3_mini(**kw)
    eng = Engine(cfg)
    eng.init_random(seed=0)
    return eng


def prompt(eng, B, text_tokens, seed=0):
    from visper_lm_amd.config import IMAGE_TOKEN_INDEX
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 30000, (B, text_tokens), generator=g)
    ids[:, 5] = IMAGE_TOKEN_INDEX
    cfg = eng.cfg
    side = cfg.cnx_image if cfg.is_convnext else cfg.vit_image
    images = torch.randn(B, 3, side, side, generator=g).to(torch.bfloat16).cuda()
    return ids, images


def time_decode(eng, B, new, text_tokens, use_graph, kv=None, wide=None):
    from visper_lm_amd import decode
    ids, images = prompt(eng, B, text_tokens)
    sess = decode.DecodeSession(eng, kv_cache_dtype=kv)
    sess.use_graph = use_graph
    sess.wide_gemm = wide
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logits = sess.prefill(ids, None, images, None, new + 1)
    torch.cuda.synchronize()
    prefill_ms = (time.perf_counter() - t0) * 1e3
    tok = torch.argmax(logits, -1)
    logits = sess.step(tok)                                   # first step: capture (graph) / warm-up (eager), not timed
    tok = torch.argmax(logits, -1)
    torch.cuda.synchronize()
    enq = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(new - 1):
        h0 = time.perf_counter()
        logits = sess.step(tok)
        enq.append((time.perf_counter() - h0) * 1e3)
        tok = torch.argmax(logits, -1)                       # on the device: no host round trip inside the timed loop
    e1.record()
    torch.cuda.synchronize()
    per_tok = e0.elapsed_time(e1) / (new - 1)
    enq.sort()
    return dict(B=B, prompt_rows=int(sess.cache.lens_host.max()) - new, prefill_ms=round(prefill_ms, 2), ms_per_token=round(per_tok, 4),
                host_enqueue_ms_per_token_median=round(enq[len(enq) // 2], 4), graph=use_graph, tokens_timed=new - 1,
                kv_cache_bytes=int(sess.cache.nbytes))


def fp8_legs(eng, B, new, text_tokens, repeats, use_graph):
    """bf16 leg and fp8 leg alternately on the quantised engine -> dict with every run, the medians, the bf16 spread and the ratio"""
    fq = eng.fq
    assert fq is not None
    legs = {"bf16": [], "fp8": []}
    for _ in range(repeats):
        for leg in ("bf16", "fp8"):
            eng.fq = None if leg == "bf16" else fq
            try:
                r = time_decode(eng, B, new, text_tokens, use_graph)
            finally:
                eng.fq = fq
            r["weights"] = leg
            legs[leg].append(r)
            print(json.dumps(r), flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    tb, t8 = [r["ms_per_token"] for r in legs["bf16"]], [r["ms_per_token"] for r in legs["fp8"]]
    spread = max(tb) - min(tb)
    return dict(B=B, graph=use_graph, repeats=repeats, bf16_ms_per_token=tb, fp8_ms_per_token=t8, bf16_median=med(tb), fp8_median=med(t8),
                bf16_spread=round(spread, 4), fp8_over_bf16=round(med(t8) / med(tb), 4), gain_ms=round(med(tb) - med(t8), 4),
                gain_exceeds_bf16_spread=bool(med(tb) - med(t8) > spread), runs=legs["bf16"] + legs["fp8"])


def mxfp4_legs(eng, fq8, B, new, text_tokens, repeats, use_graph):
    """bf16, fp8 and mxfp4 legs alternately on the engine quantised to mxfp4 -> dict with every run, the medians and the verdict"""
    fq4 = eng.fq
    assert fq4 is not None and eng.fq_format == "mxfp4"
    copies = {"bf16": (None, None), "fp8": (fq8, "e4m3"), "mxfp4": (fq4, "mxfp4")}
    legs = {k: [] for k in copies}
    for _ in range(repeats):
        for leg, (fq, fmt) in copies.items():
            eng.fq, eng.fq_format = fq, fmt
            try:
                r = time_decode(eng, B, new, text_tokens, use_graph)
            finally:
                eng.fq, eng.fq_format = fq4, "mxfp4"
            r["weights"] = leg
            legs[leg].append(r)
            print(json.dumps(r), flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    t = {k: [r["ms_per_token"] for r in v] for k, v in legs.items()}
    gain = max(t["mxfp4"]) < min(t["fp8"])
    return dict(B=B, graph=use_graph, repeats=repeats, bf16_ms_per_token=t["bf16"], fp8_ms_per_token=t["fp8"], mxfp4_ms_per_token=t["mxfp4"],
                bf16_median=med(t["bf16"]), fp8_median=med(t["fp8"]), mxfp4_median=med(t["mxfp4"]),
                mxfp4_over_fp8=round(med(t["mxfp4"]) / med(t["fp8"]), 4), mxfp4_over_bf16=round(med(t["mxfp4"]) / med(t["bf16"]), 4),
                slowest_mxfp4=max(t["mxfp4"]), fastest_fp8=min(t["fp8"]), verdict="gain" if gain else "no gain",
                runs=legs["bf16"] + legs["fp8"] + legs["mxfp4"])


def kv_legs(eng, weights, B, new, text_tokens, repeats, use_graph):
    """bf16-cache and fp8-cache legs alternately on one engine -> dict with every run, the cache bytes of both legs, the medians, the verdict"""
    names = {"bf16": "bf16", "fp8": "fp8_e4m3"}
    legs = {k: [] for k in names}
    for _ in range(repeats):
        for leg, kv in names.items():
            r = time_decode(eng, B, new, text_tokens, use_graph, kv=kv)
            r.update(weights=weights, kv=leg)
            legs[leg].append(r)
            print(json.dumps(r), flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    t = {k: [r["ms_per_token"] for r in v] for k, v in legs.items()}
    gain = max(t["fp8"]) < min(t["bf16"])
    cb = {k: v[0]["kv_cache_bytes"] for k, v in legs.items()}
    return dict(B=B, graph=use_graph, repeats=repeats, weights=weights, kv_bf16_ms_per_token=t["bf16"], kv_fp8_ms_per_token=t["fp8"],
                kv_bf16_median=med(t["bf16"]), kv_fp8_median=med(t["fp8"]), kv_fp8_over_kv_bf16=round(med(t["fp8"]) / med(t["bf16"]), 4),
                slowest_kv_fp8=max(t["fp8"]), fastest_kv_bf16=min(t["bf16"]), verdict="gain" if gain else "no gain",
                kv_bf16_cache_bytes=cb["bf16"], kv_fp8_cache_bytes=cb["fp8"], kv_fp8_over_kv_bf16_bytes=round(cb["fp8"] / cb["bf16"], 4),
                runs=legs["bf16"] + legs["fp8"])


def wide_legs(eng, weights, B, new, text_tokens, repeats, use_graph):
    """wide and chunked legs alternately on one engine -> dict with every run, ms per step and tokens per second of both legs, the verdict"""
    legs = {"wide": [], "chunked": []}
    for _ in range(repeats):
        for leg in legs:
            while True:
                try:
                    r = time_decode(eng, B, new, text_tokens, use_graph, wide=None if leg == "wide" else False)
                    break
                except torch.cuda.OutOfMemoryError:
                    torch.cuda.empty_cache()
                    text_tokens = text_tokens * 3 // 4                   # the longest prompt that fits, to a quarter
                    if text_tokens < 16:
                        raise
            r.update(weights=weights, leg=leg, text_tokens=text_tokens, tokens_per_s=round(B / r["ms_per_token"] * 1e3, 1))
            legs[leg].append(r)
            print(json.dumps(r), flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    t = {k: [r["ms_per_token"] for r in v] for k, v in legs.items()}
    texts = sorted({r["text_tokens"] for v in legs.values() for r in v})
    gain = max(t["wide"]) < min(t["chunked"])
    return dict(weights=weights, B=B, a_tiles=(B + 15) // 16, graph=use_graph, repeats=repeats, prompt=f"1 image + {texts[0]} text tokens",
                same_prompt_in_every_run=len(texts) == 1, prompt_rows=legs["wide"][-1]["prompt_rows"],
                wide_ms_per_step=t["wide"], chunked_ms_per_step=t["chunked"], wide_median=med(t["wide"]), chunked_median=med(t["chunked"]),
                wide_tokens_per_s=round(B / med(t["wide"]) * 1e3, 1), chunked_tokens_per_s=round(B / med(t["chunked"]) * 1e3, 1),
                wide_over_chunked=round(med(t["wide"]) / med(t["chunked"]), 4), slowest_wide=max(t["wide"]), fastest_chunked=min(t["chunked"]),
                verdict=("same kernel" if B <= 16 else "gain" if gain else "no gain"), runs=legs["wide"] + legs["chunked"])


SELECT_LEGS = {"torch": None, "device": dict(sync_every=1), "device_k50": dict(top_k=50, repetition_penalty=1.1, sync_every=16)}


def time_select(eng, B, new, text_tokens, use_graph, leg):
    """One run of one --select leg: generate()'s per-token work of that path (decode.generate / decode._generate_device), the loop's early
    exit left out, timed over new - 1 tokens after one warm-up / capture step"""
    from visper_lm_amd import decode
    ids, images = prompt(eng, B, text_tokens)
    sess = decode.DecodeSession(eng)
    sess.use_graph = use_graph
    gen = torch.Generator(device="cuda").manual_seed(7)
    V = eng.fz["lm_head"].shape[0]
    eos, pad = [V - 1], 0
    dev = SELECT_LEGS[leg]
    torch.cuda.synchronize()
    logits = sess.prefill(ids, None, images, None, new + 1)
    enq, reads = [], 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if dev is None:
        eos_t = torch.tensor(eos, device="cuda", dtype=torch.long)
        finished = torch.zeros(B, device="cuda", dtype=torch.bool)

        def choose(logits, finished):                             # decode.generate's loop body after the step
            raw = decode.next_tokens(logits, True, 0.8, 0.9, gen).to(torch.long)
            nxt = torch.where(finished, torch.full_like(raw, pad), raw)
            finished = finished | torch.isin(nxt, eos_t)
            bool(finished.all())
            return raw, finished

        tok, finished = choose(logits, finished)
        tok, finished = choose(sess.step(tok), finished)           # first step: capture (graph) / warm-up (eager), not timed
        torch.cuda.synchronize()
        e0.record()
        for _ in range(new - 1):
            h0 = time.perf_counter()
            logits = sess.step(tok)
            tok, finished = choose(logits, finished)
            enq.append((time.perf_counter() - h0) * 1e3)
            reads += 1
        e1.record()
    else:
        sess.alloc_select(B, new + 1, eos, pad, True, 0.8, dev.get("top_k", 0), 0.9, dev.get("repetition_penalty", 1.0), gen)
        sess.select_first(logits)
        sess.step_select()
        torch.cuda.synchronize()
        e0.record()
        for i in range(new - 1):
            h0 = time.perf_counter()
            sess.step_select()
            if (i + 1) % dev["sync_every"] == 0 or i == new - 2:
                bool((sess.finished != 0).all())
                reads += 1
            enq.append((time.perf_counter() - h0) * 1e3)
        e1.record()
    torch.cuda.synchronize()
    enq.sort()
    return dict(B=B, leg=leg, graph=use_graph, text_tokens=text_tokens, prompt_rows=int(sess.cache.lens_host.max()) - new,
                ms_per_token=round(e0.elapsed_time(e1) / (new - 1), 4), host_ms_per_token_median=round(enq[len(enq) // 2], 4),
                host_reads=reads, tokens_timed=new - 1)


def select_legs(eng, B, new, text_tokens, repeats, use_graph, on_run=None):
    """the three --select legs alternately on one engine -> dict with the medians and the verdict of device against torch; on_run(r) gets
    every run as soon as it is done (the output file is rewritten with every run)"""
    legs = {k: [] for k in SELECT_LEGS}
    for _ in range(repeats):
        for leg in legs:
            while True:
                try:
                    r = time_select(eng, B, new, text_tokens, use_graph, leg)
                    break
                except torch.cuda.OutOfMemoryError:
                    torch.cuda.empty_cache()
                    text_tokens = text_tokens * 3 // 4
                    if text_tokens < 16:
                        raise
            legs[leg].append(r)
            print(json.dumps(r), flush=True)
            if on_run is not None:
                on_run(r)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    t = {k: [r["ms_per_token"] for r in v] for k, v in legs.items()}
    texts = sorted({r["text_tokens"] for v in legs.values() for r in v})
    verdict = "gain" if max(t["device"]) < min(t["torch"]) else "loss" if min(t["device"]) > max(t["torch"]) else "no difference"
    cell = dict(B=B, graph=use_graph, repeats=repeats, prompt=f"1 image + {texts[0]} text tokens", same_prompt_in_every_run=len(texts) == 1,
                sampling="do_sample, temperature 0.8, top_p 0.9", verdict_device_vs_torch=verdict,
                device_over_torch=round(med(t["device"]) / med(t["torch"]), 4), device_k50_over_torch=round(med(t["device_k50"]) / med(t["torch"]), 4))
    for k in legs:
        cell.update({f"{k}_ms_per_token": t[k], f"{k}_median": med(t[k]),
                     f"{k}_host_ms_per_token_median": med([r["host_ms_per_token_median"] for r in legs[k]])})
    return cell


def time_lookup(eng, B, new, text_tokens, use_graph, kv, n, leg, ref):
    """One leg of --lookup: `new` tokens per sequence after the prefill.  leg "plain": the one-token step (returns the tokens [B, new + n] it
    chose, the other legs' drafts); "wrong" / "true": verify steps of n drafts that are all wrong / all right."""
    from visper_lm_amd import decode
    ids, images = prompt(eng, B, text_tokens)
    V = eng.fz["embed"].shape[0]
    plain = leg == "plain"
    sess = decode.DecodeSession(eng, kv_cache_dtype=kv, lookup=0 if plain else n)
    sess.use_graph = use_graph
    total = new + n if plain else new                         # the plain leg runs n tokens on: the last verify step's drafts
    with torch.no_grad():
        logits = sess.prefill(ids, None, images, None, total + 1)
        prompt_rows = int(sess.cache.lens_host.max())
        tok = torch.argmax(logits, -1)
        toks = [tok.cpu()]
        if plain:
            toks.append(torch.argmax(sess.step(tok), -1).cpu())               # first step: capture (graph) / warm-up (eager), not timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while len(toks) < total:
                toks.append(torch.argmax(sess.step(toks[-1].cuda()), -1).cpu())          # one host read per step, as generate()'s loop
            steps, timed = total - 2, total - 2
            out = torch.stack(toks, 1)
        else:
            raw = [[int(t)] for t in toks[0]]
            drafts = torch.empty(B, n, dtype=torch.int32)

            def one_step():
                for b in range(B):
                    c = len(raw[b])
                    d = ref[b, c:c + n]
                    drafts[b] = (d if leg == "true" else (d + 1) % V).to(torch.int32)
                nxt, n_acc = sess.verify(drafts)
                for b in range(B):
                    raw[b].extend(nxt[b, :int(n_acc[b]) + 1].tolist())

            sess.feed(tok)
            one_step()                                                            # capture / warm-up, not timed
            torch.cuda.synchronize()
            first = min(len(r) for r in raw)
            t0 = time.perf_counter()
            while min(len(r) for r in raw) < new:
                one_step()
            steps, timed = sess.steps - 1, min(len(r) for r in raw) - first
            out = torch.tensor([r[:new] for r in raw])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    if not plain:
        assert torch.equal(out, ref[:, :new]), f"lookup leg {leg}: tokens differ from the plain leg's"
        assert sess.accepted == (B * n * sess.steps if leg == "true" else 0), (leg, sess.steps, sess.accepted)
    r = dict(B=B, leg=leg, n=0 if plain else n, graph=use_graph, steps_timed=steps, tokens_timed=timed, ms_per_step=round(ms / steps, 4),
             ms_per_token=round(ms / timed, 4), prompt_rows=prompt_rows, kv_cache_bytes=int(sess.cache.nbytes))
    return r, out


def lookup_legs(eng, B, new, text_tokens, repeats, use_graph, kv, n):
    """plain, always-wrong and always-right legs alternately -> dict with every run, the medians, c and the verdict"""
    legs = {"plain": [], "wrong": [], "true": []}
    ref = None
    for _ in range(repeats):
        for leg in legs:
            r, out = time_lookup(eng, B, new, text_tokens, use_graph, kv, n, leg, ref)
            if leg == "plain":
                assert ref is None or torch.equal(ref, out), "the plain leg is not reproducible"
                ref = out
            legs[leg].append(r)
            print(json.dumps(r), flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    step = {k: [r["ms_per_step"] for r in v] for k, v in legs.items()}
    per_tok = {k: [r["ms_per_token"] for r in v] for k, v in legs.items()}
    c = med(step["wrong"]) / med(step["plain"])
    gain = max(per_tok["true"]) < min(per_tok["plain"])
    return dict(B=B, n=n, graph=use_graph, repeats=repeats, plain_ms_per_step=step["plain"], verify_ms_per_step_acceptance_0=step["wrong"],
                verify_ms_per_step_full_acceptance=step["true"], plain_median=med(step["plain"]), verify_median=med(step["wrong"]),
                c=round(c, 4), break_even_accepted_drafts_per_step=round(c - 1, 4),
                full_acceptance_ms_per_token=per_tok["true"], plain_ms_per_token=per_tok["plain"],
                slowest_full_acceptance_ms_per_token=max(per_tok["true"]), fastest_plain_ms_per_token=min(per_tok["plain"]),
                verdict_at_full_acceptance="gain" if gain else "no gain",
                acceptance_0_costs=bool(min(step["wrong"]) > max(step["plain"])), runs=legs["plain"] + legs["wrong"] + legs["true"])


def weight_bytes(eng):
    cfg = eng.cfg
    H, I, L = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
    nqkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim
    dec = L * 2 * (nqkv * H + H * cfg.num_attention_heads * cfg.head_dim + 2 * I * H + H * I)
    return dec, 2 * cfg.vocab_size * H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3", choices=["llama3", "phi3"])
    ap.add_argument("--layers", type=int, default=0, help="0 = the full depth")
    ap.add_argument("--text", type=int, default=1500)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--profile", action="store_true", help="graph on only (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument("--weights", default="bf16", choices=["bf16", "fp8", "mxfp4"],
                    help="fp8: bf16 leg, then fp8 leg, on the same quantised engine; mxfp4: bf16, fp8 and mxfp4 legs on the engine quantised to mxfp4")
    ap.add_argument("--repeats", type=int, default=3, help="--weights fp8 / mxfp4: runs of each leg, alternating")
    ap.add_argument("--graph", action="store_true", help="--weights fp8 / mxfp4: time the captured step instead of eager launches")
    ap.add_argument("--kv", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: at the chosen --weights, bf16-cache and fp8-cache legs alternately on one engine, --repeats runs each")
    ap.add_argument("--lookup", type=int, default=0,
                    help="N > 0: prompt-lookup decoding with N drafts per step: plain, always-wrong and always-right legs, --repeats runs each")
    ap.add_argument("--wide", action="store_true",
                    help="wide (one call) and chunked (16-row slices) GEMM legs alternately at B = 16, 32, 64 (--batches), --repeats runs each")
    ap.add_argument("--select", action="store_true",
                    help="torch, device and device_k50 token-selection legs alternately at B = 1, 8, 64 (--batches), eager and captured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.select:
        a.out = a.out or os.path.join(ROOT, "profiles", f"decode_bench_{a.model}_select.json")
        if a.batches == "1,8":
            a.batches = "1,8,64"
    if a.wide:
        a.out = a.out or os.path.join(ROOT, "profiles", f"decode_bench_{a.model}_wide.json")
        if a.batches == "1,8":
            a.batches = "16,32,64"
    if a.lookup and not a.out:
        a.out = os.path.join(ROOT, "profiles", f"decode_bench_{a.model}_lookup.json")
    assert torch.cuda.is_available(), "decode_bench needs a GPU"
    eng = build(a.model, a.layers)
    dec_b, head_b = weight_bytes(eng)
    res = dict(model=a.model, layers=eng.cfg.num_hidden_layers, decoder_weight_gb=round(dec_b / 1e9, 3), lm_head_gb=round(head_b / 1e9, 3),
               roofline_ms_per_token_8tbps=round((dec_b + head_b) / 8e12 * 1e3, 3), runs=[])
    def write():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    if a.select:
        res.update(select=True, weights="bf16", kv="bf16", cells=[])

        def on_run(r):
            res["runs"].append(r)
            write()

        for B in [int(x) for x in a.batches.split(",")]:
            for g in ((True,) if a.graph else (False, True)):
                res["cells"].append(select_legs(eng, B, a.new, a.text, a.repeats, g, on_run))
                write()
        a.weights = a.kv = "select"                               # the other modes below do not run
    if a.wide:
        if a.weights != "bf16":
            eng.quantize_decoder(lm_head=True, fmt="e4m3" if a.weights == "fp8" else "mxfp4")
        res.update(wide=True, lm_head_quantised_with_the_decoder=True, cells=[])
        if os.path.exists(a.out):                                 # the file collects the formats: this run replaces its own cells only
            old = json.load(open(a.out))
            if old.get("wide") and old.get("model") == a.model and old.get("layers") == res["layers"]:
                res["cells"] = [c for c in old["cells"] if c["weights"] != a.weights]
                res["runs"] = [r for r in old["runs"] if r["weights"] != a.weights]
        for B in [int(x) for x in a.batches.split(",")]:
            if a.profile:                                         # kernel-trace run: the wide leg alone, eager launches
                r = time_decode(eng, B, a.new, a.text, False)
                r.update(weights=a.weights, leg="wide")
                print(json.dumps(r), flush=True)
                continue
            cell = wide_legs(eng, a.weights, B, a.new, a.text, a.repeats, a.graph)
            res["runs"] += cell.pop("runs")
            res["cells"].append(cell)
        if a.profile:
            return
        a.weights = a.kv = "wide"                                 # the other modes below do not run
    if a.lookup:
        if a.weights != "bf16":
            eng.quantize_decoder(lm_head=True, fmt="e4m3" if a.weights == "fp8" else "mxfp4")
        res.update(weights=a.weights, kv=a.kv, lookup=a.lookup, lm_head_quantised=a.weights != "bf16", cells=[])
        for B in [int(x) for x in a.batches.split(",")]:
            if B * (a.lookup + 1) > 16:
                print(f"B = {B}: skipped, {B * (a.lookup + 1)} verify rows > 16", flush=True)
                continue
            cell = lookup_legs(eng, B, a.new, a.text, a.repeats, a.graph, "fp8_e4m3" if a.kv == "fp8" else None, a.lookup)
            res["runs"] += cell.pop("runs")
            res["cells"].append(cell)
        a.weights = a.kv = "lookup"                               # the other modes below do not run
    if a.kv == "fp8":
        if a.weights != "bf16":
            eng.quantize_decoder(lm_head=True, fmt="e4m3" if a.weights == "fp8" else "mxfp4")
        cfg = eng.cfg
        res.update(weights=a.weights, kv="fp8", lm_head_quantised=a.weights != "bf16", cells=[],
                   kv_bytes_per_token_bf16=2 * 2 * cfg.num_key_value_heads * cfg.head_dim * cfg.num_hidden_layers,
                   kv_bytes_per_token_fp8=2 * cfg.num_key_value_heads * (cfg.head_dim + 4) * cfg.num_hidden_layers)
        for B in [int(x) for x in a.batches.split(",")]:
            if a.profile:                                         # kernel-trace run: the fp8-cache leg alone, captured step
                r = time_decode(eng, B, a.new, a.text, True, kv="fp8_e4m3")
                r.update(weights=a.weights, kv="fp8")
                res["runs"].append(r)
                print(json.dumps(r), flush=True)
                continue
            cell = kv_legs(eng, a.weights, B, a.new, a.text, a.repeats, a.graph)
            res["runs"] += cell.pop("runs")
            res["cells"].append(cell)
    if a.kv == "bf16" and a.weights == "fp8":
        eng.quantize_decoder(lm_head=True)
        res.update(weights="fp8", lm_head_fp8=True, fp8_roofline_ms_per_token_8tbps=round((dec_b + head_b) / 2 / 8e12 * 1e3, 3), cells=[])
        for B in [int(x) for x in a.batches.split(",")]:
            if a.profile:                                         # kernel-trace run: the fp8 leg alone, captured step
                r = time_decode(eng, B, a.new, a.text, True)
                r["weights"] = "fp8"
                res["runs"].append(r)
                print(json.dumps(r), flush=True)
                continue
            cell = fp8_legs(eng, B, a.new, a.text, a.repeats, a.graph)
            cell["fp8_weight_bytes_share_of_8tbps"] = round((dec_b + head_b) / 2 / 8e12 * 1e3 / cell["fp8_median"], 3)
            cell["bf16_weight_bytes_share_of_8tbps"] = round((dec_b + head_b) / 8e12 * 1e3 / cell["bf16_median"], 3)
            res["runs"] += cell.pop("runs")
            res["cells"].append(cell)
    if a.kv == "bf16" and a.weights == "mxfp4":
        from visper_lm_amd import ops
        eng.quantize_decoder(lm_head=True, fmt="mxfp4")
        fq8 = {k: ops.quant_rows_e4m3(eng.fz[k]) for k in eng.fq}            # e4m3 copies of the written-back weights, no second write-back
        # mxfp4 bytes per weight: half a byte of codes + one scale byte per 32
        res.update(weights="mxfp4", lm_head_mxfp4=True, mxfp4_roofline_ms_per_token_8tbps=round((dec_b + head_b) / 2 * (0.5 + 1 / 32) / 8e12 * 1e3, 3),
                   cells=[])
        for B in [int(x) for x in a.batches.split(",")]:
            if a.profile:                                         # kernel-trace run: the mxfp4 leg alone, captured step
                r = time_decode(eng, B, a.new, a.text, True)
                r["weights"] = "mxfp4"
                res["runs"].append(r)
                print(json.dumps(r), flush=True)
                continue
            cell = mxfp4_legs(eng, fq8, B, a.new, a.text, a.repeats, a.graph)
            res["runs"] += cell.pop("runs")
            res["cells"].append(cell)
    for B in ([] if a.weights != "bf16" or a.kv != "bf16" else [int(x) for x in a.batches.split(",")]):
        for g in ((True,) if a.profile else (True, False)):
            r = time_decode(eng, B, a.new, a.text, g)
            kv_bytes_per_pos = 2 * 2 * eng.cfg.num_key_value_heads * eng.cfg.head_dim * eng.cfg.num_hidden_layers
            r["kv_gb_mid_decode"] = round(B * (r["prompt_rows"] + a.new // 2) * kv_bytes_per_pos / 1e9, 3)
            r["weight_bytes_share_of_8tbps"] = round((dec_b + head_b) / 8e12 * 1e3 / r["ms_per_token"], 3)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
    print(json.dumps(res))
    write()


if __name__ == "__main__":
    main()
