"""Gradient checkpointing at full model size through the model API (random init, the step bench.py times: forward through the model
class, .loss.backward(), model.optimizer_step, zero_grad; a fresh batch of token ids per step): ms per step and the process's peak
allocation (torch.cuda.max_memory_allocated) with the switch off / "full" / "keep_attn".

One child process per leg, each under its own `timeout`.  A leg is stage:batch:mode — stage pt (configs[1]: ViT-L + Llama-3-8B, 3 heads,
S = 2048) or ift (whole LLM trainable, NTP only, S = 2048).  A leg that runs out of memory is recorded with the allocator's message and
byte count, and nothing is started after it in that run (so list a leg that is expected not to fit last).  Results are merged into --out
by leg name.  "off" legs also time Engine.train_step(batch, compute_grads=False) on the same batches: the bound the recompute's cost is
held to (that step is a superset of what is recomputed).

  python tools/checkpoint_bench.py --legs pt:8:off,pt:8:full,pt:8:keep_attn
  python tools/checkpoint_bench.py --legs pt:32:full,pt:32:off
  python tools/checkpoint_bench.py --legs ift:8:off,ift:8:full,ift:16:full,ift:16:off
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_LEGS = "pt:8:off,pt:8:full,pt:8:keep_attn,pt:32:full,ift:8:off,ift:8:full,ift:16:full,pt:32:off,ift:16:off"
MAX_ROWS = 65536          # B x S: the largest operand (gate|up, rows x 28 672 bf16) stays below the 4 GiB a buffer descriptor addresses


def run_leg(stage, B, mode, steps, warmup):
    import torch
    import bench
    from visper_lm_amd import model as M_
    from visper_lm_amd.config import llama3_8b
    assert torch.cuda.is_available(), "checkpoint_bench needs a GPU"
    dev = torch.device("cuda", 0)
    if stage == "ift":
        cfg, T = llama3_8b(aux_mode="", num_task_tokens=0, train_llm=True), 1473
        mcls, ccls = M_.LlavaLlamaForCausalLM, M_.LlavaConfig
    else:
        cfg, T = llama3_8b(), 1449
        cfg.depth_decoder = True
        mcls, ccls = M_.OlaLlavaLlamaForCausalLM, M_.OlaLlavaLlamaConfig
    S = 2048
    assert B * S <= MAX_ROWS and B * S * 2 * cfg.intermediate_size * 2 < 2 ** 32, "beyond what one buffer descriptor addresses"
    cd = cfg.to_dict()
    for k in getattr(ccls, "STORED_KEYS_IGNORED", ()):
        cd.pop(k, None)
    mcfg = ccls(**cd)
    mcfg.reference_outputs = False
    res = dict(leg=f"{stage}:{B}:{mode}", stage=stage, batch=B, S=S, mode=mode, steps=steps, warmup=warmup)
    try:
        model = mcls(mcfg, device=dev, init="random", seed=0)
        if mode != "off":
            mcfg.gradient_checkpointing = mode
            model.gradient_checkpointing_enable()
        eng = model._get_engine()
        cfg = eng.cfg
        pool = [bench.make_batch(cfg, B, T, 1000 * j, dev) for j in range(2)]
        gi = torch.Generator().manual_seed(4321)
        fresh = []
        for j in range(warmup + steps):
            b = dict(pool[j % len(pool)])
            ids = torch.randint(0, 1000, (B, T), generator=gi)
            ids[:, cfg.num_sys_tokens] = -200
            lab = ids.clone()
            lab[:, :cfg.num_sys_tokens + 7] = -100
            b["input_ids"], b["labels"], b["images_resident"] = ids, lab, True
            fresh.append(b)
        torch.cuda.synchronize()
        res["weights_gb"] = round(torch.cuda.memory_allocated() / 1e9, 2)

        def step(b):
            out = model(**b)
            out.loss.backward()
            model.optimizer_step(lr=1e-3)
            model.zero_grad(set_to_none=True)
            return out.loss.detach()
        for b in fresh[:warmup]:
            loss = step(b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in fresh[warmup:]:
            loss = step(b)
        torch.cuda.synchronize()
        res["ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / steps, 2)
        res["peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
        res["loss"] = float(loss)
        res["last_fold"] = bool(eng.last_fold)
        if mode == "off":
            eb = [dict(input_ids=b["input_ids"], labels=b["labels"], images=b["images"], images_resident=True,
                       **{k: v for k, v in b.items() if k.endswith("_target") or k.endswith("_mask")}) for b in fresh[warmup:]]
            eng.train_step(eb[0], compute_grads=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in eb:
                eng.train_step(b, compute_grads=False)
            torch.cuda.synchronize()
            res["fwd_only_ms"] = round((time.perf_counter() - t0) * 1e3 / len(eb), 2)
    except torch.OutOfMemoryError as e:
        msg = str(e)
        m = re.search(r"Tried to allocate ([0-9.]+) ([KMG]iB)", msg)
        res["oom"] = msg.splitlines()[0][:400]
        res["oom_request_bytes"] = int(float(m.group(1)) * {"KiB": 2 ** 10, "MiB": 2 ** 20, "GiB": 2 ** 30}[m.group(2)]) if m else None
        res["allocated_gb_at_oom"] = round(torch.cuda.memory_allocated() / 1e9, 2)
        res["peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=DEFAULT_LEGS, help="comma list of stage:batch:mode (stage pt | ift, mode off | full | keep_attn)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        stage, B, mode = a.child.split(":")
        return run_leg(stage, int(B), mode, a.steps, a.warmup)
    results = {}
    if os.path.exists(a.out):
        results = {r["leg"]: r for r in json.load(open(a.out))["legs"]}
    for leg in a.legs.split(","):
        stage, B, mode = leg.split(":")
        assert stage in ("pt", "ift") and mode in ("off", "full", "keep_attn") and int(B) * 2048 <= MAX_ROWS, leg
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg,
                            "--steps", str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
        r = json.loads(lines[-1][4:]) if lines else dict(leg=leg, failed=True, stderr_tail=p.stderr[-800:])
        r["exit_code"] = p.returncode
        results[leg] = r
        print(json.dumps(r), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(dict(tool="tools/checkpoint_bench.py", legs=list(results.values())), fh, indent=1)
            fh.write("\n")
        if p.returncode != 0 or "oom" in r or not lines:
            print(f"checkpoint_bench: leg {leg} did not complete (exit {p.returncode}): nothing is started after it", flush=True)
            sys.exit(0 if (p.returncode == 0 and lines) else 1)       # a recorded out-of-memory leg is a result, anything else a failure


if __name__ == "__main__":
    main()
