"""``llama`` plugin: ``POST /generate`` on Llama-3-8B, tensor-parallel over the node (config 5).

Request: ``{"prompt": str | "input_ids": [int], "max_new_tokens": int, "top_k": int,
"temperature": float, "seed": int}``.  With ``CONTINUOUS_BATCHING`` (default) requests join and
leave the running decode batch at every step (``models/llama_serving.py``); otherwise
concurrent requests are micro-batched (same batcher as ``/predict``), right-padded and generated
together (batched prefill with per-sequence lengths, then lockstep decode steps).

Multi-GPU: rank 0 owns HTTP.  For each batch it broadcasts a small command header and the
token ids to the other ranks (X5); every rank then runs the same TP forward, and the
top-k candidate merge makes the sampled token identical on all ranks, so no per-token
broadcast is needed.  Followers sit in :meth:`follower_loop` until rank 0 sends STOP.
"""
from __future__ import annotations

import logging
import threading
from typing import Any, Dict, List, Tuple

import torch

from ..models.llama_serving import OP_GENERATE, OP_ITER, OP_STOP
from .base import ModelPlugin, PluginContext, register

logger = logging.getLogger("mlsamd.plugin")


@register("llama")
class LlamaPlugin(ModelPlugin):
    name = "llama"
    batched = True
    task = "generate"

    def __init__(self):
        self.model = None
        self.tok = None
        self.ctx = None
        self.comm_dev = None
        self.prefill_chunk = 0
        self.speculate, self.speculate_ngram = 0, 3
        self.speculate_device = False
        self.prefix_cache = False
        self.adapters: Dict[str, int] = {}  # MODEL_CONFIG lora: adapter name -> index
        self.kv_pages = 0
        self._lock = threading.Lock()

    def init(self, ctx: PluginContext) -> None:
        from ..models import llama

        self.ctx = ctx
        s = ctx.settings
        extra = s.model_yaml() if hasattr(s, "model_yaml") else {}
        weight_dtype = self.parse_weight_dtype(extra)  # before any weight is read or allocated
        self.speculate, self.speculate_ngram = self.parse_speculate(extra)
        self.speculate_device = self.parse_speculate_device(extra, self.speculate)
        self.prefix_cache = self.parse_prefix_cache(extra)
        lora_paths, lora_kw = self.parse_lora(extra, self.prefix_cache)
        size = extra.get("config", "8b")
        cfg = llama.LLAMA3_8B if size == "8b" else llama.tiny_config(**extra.get("overrides", {}))
        tp = ctx.world_size if int(s.TP) > 1 else 1
        if tp > 1 and ctx.world_size != tp:
            raise RuntimeError(f"TP={s.TP} needs WORLD_SIZE={tp}")
        on_gpu = torch.cuda.is_available() and bool(ctx.devices)
        dev = ctx.devices[0] if on_gpu else "cpu"
        backend = s.BACKEND if (on_gpu and s.BACKEND == "fused") else "reference"
        self.comm_dev = torch.device(dev)
        # every TP rank reads just its own slices from the checkpoint (no weight broadcast needed)
        source = llama.CheckpointSource(s.WEIGHTS, device=dev) if s.WEIGHTS else None
        params = llama.init_llama_shard(cfg, tp, ctx.rank, int(s.SEED), device=dev, source=source)
        max_batch, max_seq = int(s.MAX_BATCH) or 32, int(extra.get("max_seq", 2048))
        kv_dtype = str(extra.get("kv_dtype", "bf16"))  # MODEL_CONFIG kv_dtype: bf16 | fp8 (e4m3 KV cache)
        # MODEL_CONFIG prefill_chunk: N > 0 = chunked prefill, N prompt positions per serving iteration
        self.prefill_chunk = int(extra.get("prefill_chunk", 0) or 0)
        if self.prefill_chunk < 0:
            raise ValueError(f"prefill_chunk must be >= 0, got {self.prefill_chunk}")
        # MODEL_CONFIG kv_prefill: rows | cache (fp8 only: prefill attends the e4m3 cache rows, LlamaTP(kv_prefill=))
        kv_prefill = str(extra.get("kv_prefill", "rows"))
        if self.prefill_chunk and kv_dtype == "fp8" and kv_prefill != "cache":  # LlamaTP.check_prefill_chunk's rule
            raise ValueError("prefill_chunk is not available with kv_dtype: fp8 (a chunk would attend e4m3 context "
                             "rows where one-shot prefill attends unquantised ones)")
        kv_pages = self._kv_pages(extra.get("kv_pages", 0), cfg, tp, max_batch, max_seq, dev, backend, kv_dtype)
        if tp > 1 and kv_pages:  # the scheduler replays rank 0's admissions: every pool must be equal
            from ..parallel import dist as mdist

            kv_pages = int(-mdist.max_over_ranks(-float(kv_pages)))
        self.model = llama.LlamaTP(params, cfg, tp=tp, rank=ctx.rank, comm=llama.TPComm(None, tp, device=dev), backend=backend,
                                   device=dev, max_batch=max_batch, max_seq=max_seq, kv_pages=kv_pages,
                                   kv_dtype=kv_dtype, weight_dtype=weight_dtype, kv_prefill=kv_prefill, lora=lora_kw)
        for index, (name, path) in enumerate(lora_paths.items()):  # every rank reads the adapter and keeps its B rows
            from ..utils.checkpoint import load_lora_adapter

            tensors, acfg = load_lora_adapter(path, cfg.layers)
            self.model.load_adapter(index, tensors, acfg)
            self.adapters[name] = index
        if self.speculate:  # refused at start-up on the lockstep path too (the engine below checks for itself)
            self.model.check_speculate(self.speculate)
        if self.speculate_device:  # no device loop (reference backend, CPU, graphs off ...): refused, nothing falls back
            self.model.check_spec_device(self.speculate)
        if self.prefix_cache:  # no paged KV, fp8 KV with kv_prefill: rows, row-major cache, head_dim != 128: refused, nothing falls back
            self.model.check_prefix_cache()
            if not bool(getattr(s, "CONTINUOUS_BATCHING", True)):
                raise ValueError("prefix_cache needs continuous batching (the lockstep generate path has no page sharing)")
        self.tok = llama.LlamaTokenizer(cfg, extra.get("tokenizer_file"))
        self.cfg = cfg
        self.engine = None
        if bool(getattr(s, "CONTINUOUS_BATCHING", True)):
            from ..models.llama_serving import ContinuousLlama

            self.engine = ContinuousLlama(self.model, max_queue=int(s.MAX_QUEUE), channel=self if tp > 1 else None,
                                          prefill_chunk=self.prefill_chunk, speculate=self.speculate,
                                          drafter=self._drafter(), prefix_cache=self.prefix_cache,
                                          **self._spec_device_kw())
            if ctx.rank == 0:
                self.engine.start()
        self.kv_pages = kv_pages
        logger.info("llama ready: tp=%d rank=%d backend=%s device=%s kv_dtype=%s kv_prefill=%s kv_bytes_per_token=%d "
                    "weight_dtype=%s layer_weight_bytes=%d prefix_cache=%s", tp, ctx.rank, backend, dev, kv_dtype,
                    kv_prefill, self.kv_page_bytes(cfg, tp, backend, kv_dtype) // 64, weight_dtype,
                    self.model.layer_weight_bytes(), self.prefix_cache)

    @staticmethod
    def parse_weight_dtype(extra: dict) -> str:
        """MODEL_CONFIG ``weight_dtype``: ``bf16`` (default) | ``int4`` (W4A16 layer projections) | ``w8a8``
        (e4m3 weights and activations on the block-scaled MFMA, at every batch size;
        :class:`~..models.llama.LlamaTP`)."""
        wd = str(extra.get("weight_dtype", "bf16"))
        if wd not in ("bf16", "int4", "w8a8"):
            raise ValueError(f"weight_dtype must be 'bf16', 'int4' or 'w8a8', got {wd!r}")
        return wd

    @staticmethod
    def parse_lora(extra: dict, prefix_cache: bool = False):
        """MODEL_CONFIG ``lora: {name: PEFT directory, ...}`` (+ optional ``lora_max_rank``, default 64):
        ``(paths, LlamaTP's lora=...)``, ``({}, None)`` without adapters.  Refused together with
        ``prefix_cache: true`` (cached pages hold adapter-specific K / V)."""
        paths = extra.get("lora") or {}
        if not isinstance(paths, dict) or not all(isinstance(k, str) and isinstance(v, str) for k, v in paths.items()):
            raise ValueError(f"lora must map adapter names to directories, got {paths!r}")
        if not paths:
            return {}, None
        if prefix_cache:
            raise ValueError("prefix_cache: true is not available together with lora adapters (cached pages hold "
                             "adapter-specific K / V; the prefix index is not keyed by adapter)")
        return dict(paths), {"max_adapters": len(paths), "max_rank": int(extra.get("lora_max_rank", 64))}

    @staticmethod
    def parse_prefix_cache(extra: dict) -> bool:
        """MODEL_CONFIG ``prefix_cache``: ``true`` | ``false`` (default): share the KV pages of repeated
        prompt prefixes between requests (models/prefix_cache.py; needs ``kv_pages``)."""
        v = extra.get("prefix_cache", False)
        if not isinstance(v, bool):
            raise ValueError(f"prefix_cache must be true or false, got {v!r}")
        return v

    @staticmethod
    def parse_speculate(extra: dict):
        """MODEL_CONFIG ``speculate``: K draft tokens per sequence and decode step, an integer in [0, 7]
        (default 0 = off), and ``speculate_ngram``: the longest n-gram prompt lookup matches (default 3)."""
        out = []
        for key, default, lo, hi in (("speculate", 0, 0, 7), ("speculate_ngram", 3, 1, 64)):
            v = extra.get(key, default)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"{key} must be an integer in [{lo}, {hi}], got {v!r}")
            out.append(v)
        return tuple(out)

    @staticmethod
    def parse_speculate_device(extra: dict, speculate: int) -> bool:
        """MODEL_CONFIG ``speculate_device``: ``true`` | ``false`` (default): with ``speculate``, verify
        steps draft (prompt lookup, ``speculate_ngram``) and accept on device inside the captured step
        (models/llama_serving.py); needs ``speculate >= 1``."""
        v = extra.get("speculate_device", False)
        if not isinstance(v, bool):
            raise ValueError(f"speculate_device must be true or false, got {v!r}")
        if v and not speculate:
            raise ValueError("speculate_device needs speculate >= 1")
        return v

    def _spec_device_kw(self) -> dict:
        """``spec_device`` / ``spec_ngram`` of the engine and of ``generate`` (nothing when off)."""
        return dict(spec_device=True, spec_ngram=(self.speculate_ngram, 1)) if self.speculate_device else {}

    def _drafter(self):
        if not self.speculate or self.speculate_device:  # on device the drafter is the kernel's prompt lookup
            return None
        from ..models.speculative import make_prompt_lookup

        return make_prompt_lookup(max_ngram=self.speculate_ngram)

    @staticmethod
    def kv_page_bytes(cfg, tp: int, backend: str = "fused", kv_dtype: str = "bf16") -> int:
        """Bytes of one 64-row KV page over all layers of one rank, K and V: bf16 rows on the fused
        backend, fp32 on the reference backend (which keeps dequantised rows, whatever ``kv_dtype``),
        and with ``kv_dtype="fp8"`` on the fused backend one e4m3 byte per element plus one fp32
        scale per (row, KV head)."""
        from ..models.llama import shard_dims

        hkv = shard_dims(cfg, tp, 0).hkv
        if backend != "fused":
            row = cfg.head_dim * 4
        elif kv_dtype == "fp8":
            row = cfg.head_dim + 4
        else:
            row = cfg.head_dim * 2
        return cfg.layers * 2 * 64 * hkv * row

    @staticmethod
    def _kv_pages(spec, cfg, tp, max_batch, max_seq, dev, backend: str = "fused", kv_dtype: str = "bf16") -> int:
        """MODEL_CONFIG ``kv_pages``: 0 = per-slot caches (``max_batch x max_seq`` rows), N = a
        shared pool of N 64-row pages, ``auto`` = as many pages as half the free HBM holds, capped
        at what ``max_batch`` full-length sequences could use (+ the scratch page).  Under TP the
        ranks then agree on the minimum (rank 0's admissions are replayed on every rank)."""
        if spec in (0, "0", None, ""):
            return 0
        full = max_batch * -(-max_seq // 64) + 1
        if str(spec) != "auto":
            return int(spec)
        page_bytes = LlamaPlugin.kv_page_bytes(cfg, tp, backend, kv_dtype)
        if torch.device(dev).type != "cuda":
            return full
        free, _total = torch.cuda.mem_get_info(torch.device(dev))
        return LlamaPlugin.kv_pages_for(free, page_bytes, full)

    @staticmethod
    def kv_pages_for(free_bytes: int, page_bytes: int, full: int) -> int:
        """``kv_pages: auto``: the pages half of ``free_bytes`` holds, at least 2, at most ``full``."""
        return max(2, min(full, int(free_bytes * 0.5) // page_bytes))

    # ------------------------------------------------------------------ request path
    def prepare_generate(self, req: dict) -> Tuple[List[int], Any]:
        from ..models.llama import GenParams

        if "input_ids" in req:
            ids = [int(i) for i in req["input_ids"]]
        else:
            ids = self.tok.encode(str(req["prompt"]))
        gp = GenParams(max_new_tokens=int(req.get("max_new_tokens", self.ctx.settings.MAX_NEW_TOKENS)),
                       top_k=int(req.get("top_k", 1)), temperature=float(req.get("temperature", 1.0)),
                       seed=int(req.get("seed", 0)), adapter=self.adapter_index(req.get("adapter")))
        if not ids:
            raise ValueError("empty prompt")
        if gp.max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        return ids, gp

    def adapter_index(self, name) -> int:
        """``"adapter"`` of a request -> the model's adapter index (absent: -1, the base model); an unknown
        name is a ``ValueError``, as an empty prompt is."""
        if name is None:
            return -1
        if not isinstance(name, str) or name not in self.adapters:
            raise ValueError(f"unknown adapter {name!r} (configured: {sorted(self.adapters)})")
        return self.adapters[name]

    def submit_generate(self, sample):
        """Continuous batching: enqueue into the scheduler; a concurrent.futures.Future of the
        ``(prompt_len, tokens)`` pair :meth:`finish_generate` formats (None: no engine)."""
        if self.engine is None:
            return None
        ids, gp = sample
        fut = self.engine.submit(ids, gp)
        import concurrent.futures as cf

        out: cf.Future = cf.Future()

        def done(f, n=len(ids)):
            if f.exception() is not None:
                out.set_exception(f.exception())
            else:
                out.set_result((n, f.result()))

        fut.add_done_callback(done)
        return out

    def finish_generate(self, out: Any) -> dict:
        prompt_len, toks = out
        eos = set(self.cfg.eos_ids)
        cut = next((i + 1 for i, t in enumerate(toks) if t in eos), len(toks))
        toks = toks[:cut]
        return {"token_ids": toks, "text": self.tok.decode(toks), "num_tokens": len(toks), "prompt_tokens": prompt_len}

    def replicas(self):
        def run_batch(samples):
            groups: Dict[tuple, List[int]] = {}
            for i, (_ids, gp) in enumerate(samples):
                if not isinstance(gp.adapter, int):
                    raise ValueError(f"a request names one adapter index, got {gp.adapter!r}")
                groups.setdefault((gp.top_k, gp.temperature, gp.seed, gp.adapter), []).append(i)
            results: List[Any] = [None] * len(samples)
            for _key, members in groups.items():
                ids_l = [samples[i][0] for i in members]
                gp = samples[members[0]][1]
                from ..models.llama import GenParams

                gpg = GenParams(max(samples[i][1].max_new_tokens for i in members), gp.top_k, gp.temperature, gp.seed,
                                gp.adapter)
                toks = self._generate_batch(ids_l, gpg)
                for j, i in enumerate(members):
                    results[i] = (len(ids_l[j]), toks[j][: samples[i][1].max_new_tokens])
            return results

        return [run_batch]

    # ------------------------------------------------------------------ lockstep execution
    def _broadcast_cmd(self, op: int, ids: torch.Tensor = None, lens: torch.Tensor = None, gp=None) -> None:
        import torch.distributed as dist

        if self.model.tp == 1:
            return
        hdr = torch.zeros(8, dtype=torch.int64, device=self.comm_dev)
        if op == OP_GENERATE:
            if not isinstance(gp.adapter, int):  # one adapter per lockstep batch (run_batch groups by it)
                raise ValueError(f"the lockstep header carries one adapter index, got {gp.adapter!r}")
            hdr[:] = torch.tensor([op, ids.shape[0], ids.shape[1], gp.max_new_tokens, gp.top_k,
                                   int(gp.temperature * 1000), gp.seed, int(gp.adapter)])
        dist.broadcast(hdr, src=0)
        if op == OP_GENERATE:
            dist.broadcast(ids.to(self.comm_dev), src=0)
            dist.broadcast(lens.to(self.comm_dev), src=0)

    def _generate_batch(self, ids_l: List[List[int]], gp) -> List[List[int]]:
        S = max(len(t) for t in ids_l)
        B = len(ids_l)
        ids = torch.zeros(B, S, dtype=torch.int32)
        for i, t in enumerate(ids_l):
            ids[i, : len(t)] = torch.tensor(t, dtype=torch.int32)
        lens = torch.tensor([len(t) for t in ids_l], dtype=torch.int32)
        with self._lock:
            self._broadcast_cmd(OP_GENERATE, ids, lens, gp)
            out = self.model.generate(ids, lens, gp, prefill_chunk=self.prefill_chunk, speculate=self.speculate,
                                      drafter=self._drafter(), **self._spec_device_kw())
        return out.cpu().tolist()

    # ---- the continuous engine's TP control channel (models/llama_serving.py ContinuousLlama):
    # explicit headers only when no decode step carried one; admissions only when there are any
    def send_header(self, admit) -> None:
        """Rank 0: one iteration's header (None = stop), then its admissions when it has any."""
        import torch.distributed as dist

        hdr = torch.zeros(8, dtype=torch.int64, device=self.comm_dev)
        if admit is None:
            dist.broadcast(hdr, src=0)  # OP_STOP
            return
        n = len(admit)
        S = max((len(a.ids) for a in admit), default=0)
        hdr[:3] = torch.tensor([OP_ITER, n, S])
        dist.broadcast(hdr, src=0)
        if n:
            self.send_admissions(admit)

    def send_admissions(self, admit) -> None:
        """Rank 0: the admitted sequences' slot / length / sampling parameters and prompt ids."""
        import torch.distributed as dist

        n = len(admit)
        S = max(len(a.ids) for a in admit)
        meta = torch.tensor([[a.slot, len(a.ids), a.gp.max_new_tokens, a.gp.top_k, round(a.gp.temperature * 1000),
                              a.gp.seed, int(a.gp.adapter)] for a in admit], dtype=torch.int64, device=self.comm_dev)
        ids = torch.zeros(n, S, dtype=torch.int64, device=self.comm_dev)
        for j, a in enumerate(admit):
            ids[j, : len(a.ids)] = torch.tensor(a.ids, dtype=torch.int64)
        dist.broadcast(meta, src=0)
        dist.broadcast(ids, src=0)

    def recv_header(self):
        """Followers: (op, admissions, longest prompt) of rank 0's explicit header."""
        import torch.distributed as dist

        hdr = torch.zeros(8, dtype=torch.int64, device=self.comm_dev)
        dist.broadcast(hdr, src=0)
        op, n, S = hdr[:3].tolist()
        return op, n, S

    def recv_admissions(self, n: int, S: int):
        """Followers: the ``n`` sequences rank 0 admits this iteration (prompts padded to ``S``)."""
        import torch.distributed as dist

        from ..models.llama import GenParams
        from ..models.llama_serving import _Seq

        meta = torch.zeros(n, 7, dtype=torch.int64, device=self.comm_dev)
        ids = torch.zeros(n, S, dtype=torch.int64, device=self.comm_dev)
        dist.broadcast(meta, src=0)
        dist.broadcast(ids, src=0)
        admit = []
        ids_l = ids.tolist()
        for j, (slot, ln, mnt_j, topk_j, temp_j, seed_j, ad_j) in enumerate(meta.tolist()):
            seq = _Seq(ids_l[j][:ln], GenParams(mnt_j, topk_j, temp_j / 1000.0, seed_j, ad_j), None)
            seq.slot = slot
            admit.append(seq)
        return admit

    def _broadcast_iter(self, admit) -> None:
        """Rank 0, continuous mode, one header per iteration (the legacy hook form)."""
        self.send_header(admit)

    def follower_loop(self) -> int:
        """Ranks > 0: execute rank 0's generate commands until STOP."""
        import torch.distributed as dist

        import time

        from ..models.llama import GenParams

        if self.engine is not None:  # continuous batching: the engine's own follow loop (headers
            try:                     # carried by the decode steps where possible)
                return self.engine.follow()
            finally:
                self.follower_stats = dict(self.engine.follower_stats, **self.engine.proto)
        # per-iteration host cost of following (X5): the header broadcast + its host read, and the
        # iteration itself -- in the worker's info dump (tests/llama_tp_worker.py) and /info
        st = self.follower_stats = {"iters": 0, "hdr_s": 0.0, "hdr_max_s": 0.0, "iter_s": 0.0}
        while True:
            t0 = time.perf_counter()
            hdr = torch.zeros(8, dtype=torch.int64, device=self.comm_dev)
            dist.broadcast(hdr, src=0)
            op, B, S, mnt, topk, temp, seed, adapter = hdr.tolist()
            dt = time.perf_counter() - t0
            st["hdr_s"] += dt
            st["hdr_max_s"] = max(st["hdr_max_s"], dt)
            if op == OP_STOP:
                logger.info("rank %d: stop", self.ctx.rank)
                return 0
            if op == OP_ITER:  # continuous batching: replay rank 0's iteration
                from ..models.llama_serving import _Seq

                admit = []
                if B:
                    meta = torch.zeros(B, 7, dtype=torch.int64, device=self.comm_dev)
                    ids = torch.zeros(B, S, dtype=torch.int64, device=self.comm_dev)
                    dist.broadcast(meta, src=0)
                    dist.broadcast(ids, src=0)
                    for j, (slot, n, mnt_j, topk_j, temp_j, seed_j, ad_j) in enumerate(meta.tolist()):
                        seq = _Seq(ids[j, :n].tolist(), GenParams(mnt_j, topk_j, temp_j / 1000.0, seed_j, ad_j), None)
                        seq.slot = slot
                        admit.append(seq)
                t1 = time.perf_counter()
                self.engine.run_iteration(admit)  # same failure handling / health checks as rank 0
                st["iter_s"] += time.perf_counter() - t1
                st["iters"] += 1
                continue
            ids = torch.zeros(B, S, dtype=torch.int32, device=self.comm_dev)
            lens = torch.zeros(B, dtype=torch.int32, device=self.comm_dev)
            dist.broadcast(ids, src=0)
            dist.broadcast(lens, src=0)
            self.model.generate(ids, lens, GenParams(mnt, topk, temp / 1000.0, seed, adapter),
                                prefill_chunk=self.prefill_chunk, speculate=self.speculate, drafter=self._drafter(),
                                **self._spec_device_kw())

    def close(self) -> None:
        if self.engine is not None and self.ctx.rank == 0:
            self.engine.stop()  # in TP mode its scheduler announces STOP to the followers
            if self.model.tp > 1:
                return
        if self.model is not None and self.model.tp > 1 and self.ctx.rank == 0:
            try:
                self._broadcast_cmd(OP_STOP)
            except Exception as e:  # followers may already be gone
                logger.warning("stop broadcast failed: %s", e)

    def describe(self) -> dict:
        d = super().describe()
        if self.model is not None:
            d.update({"tp": self.model.tp, "backend": self.model.backend, "max_batch": self.model.max_batch,
                      "max_seq": self.model.max_seq, "speculate": self.speculate,
                      "speculate_ngram": self.speculate_ngram, "speculate_device": self.speculate_device,
                      "prefix_cache": self.prefix_cache, "adapters": sorted(self.adapters),
                      "kv_dtype": self.model.kv_dtype, "kv_prefill": self.model.kv_prefill,
                      "kv_pages": self.kv_pages, "prefill_chunk": self.prefill_chunk})
        return d
