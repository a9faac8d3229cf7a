"""Llama-3-8B generation with Megatron-style tensor parallelism (BASELINE.json config 5, P3/P6
of SURVEY.md §2.E.3).  No reference counterpart (the reference model is a stub).

Sharding per rank r of ``tp`` (one process per GPU, RCCL over xGMI):
  * column-parallel: fused QKV (``hq = heads/tp`` query heads, ``hkv = kv_heads/tp`` KV heads),
    fused gate/up (``I/tp`` rows each, interleaved for the SiLU-mul epilogue);
  * row-parallel: o_proj and down_proj -> one all-reduce each per layer (X2, 2 x 32 / forward);
  * vocab-parallel embedding (out-of-shard ids give zero rows, then all-reduce, X3) and lm_head
    (each rank takes a local top-k of its 16032-row shard; ranks all-gather only k candidates
    per sequence and merge -- X4 -- instead of gathering 128256 logits).
The residual add is fused into the RMSNorm kernel AFTER the all-reduce (adding the replicated
residual before it would count it ``tp`` times).

Two backends with identical structure and communication:
  * ``reference``: plain PyTorch fp32 math on bf16 weights (runs on CPU with gloo -- the TP
    logic is tested there against TP=1);
  * ``fused``: the CDNA4 kernels (MFMA GEMMs with fused SiLU-mul, RMSNorm+residual, RoPE,
    KV-cache append, MFMA flash-attention prefill, split-KV decode attention, top-k).
Weights are random-init (std 0.02) and generated per tensor from a (seed, name) generator on
the target device, then sliced to the rank's shard -- every rank gets exactly the slice of the
same full model, without any rank materialising the whole 8B model.
"""
from __future__ import annotations

import hashlib
import os
import re
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.distributed as dist
import torch.nn.functional as F

from ..ops import reference as R
from ..utils import tracing
from .llama_route import ProjTiers, StepRoute, proj_tiers, step_route

# int32 words of the serving loop's control row (op, admissions, longest prompt, iteration check):
# rank 0's next-iteration header, carried by the decode step's X4 gather (serve_graph)
CTL_WORDS = 4


@dataclass
class LlamaConfig:
    vocab: int = 128256
    hidden: int = 4096
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    head_dim: int = 128
    intermediate: int = 14336
    rope_theta: float = 500000.0
    eps: float = 1e-5
    bos_id: int = 128000
    eos_ids: Tuple[int, ...] = (128001, 128009)


LLAMA3_8B = LlamaConfig()


def tiny_config(**kw) -> LlamaConfig:
    base = dict(vocab=2048, hidden=256, layers=2, heads=8, kv_heads=4, head_dim=32, intermediate=512, bos_id=1,
                eos_ids=(2,))
    base.update(kw)
    return LlamaConfig(**base)


@dataclass
class ShardDims:
    tp: int
    rank: int
    hq: int
    hkv: int
    inter: int
    vocab_shard: int
    vocab_lo: int

    @property
    def qkv_rows(self) -> int:
        return 0


def shard_dims(cfg: LlamaConfig, tp: int, rank: int) -> ShardDims:
    if cfg.heads % tp or cfg.intermediate % tp:
        raise ValueError(f"tp={tp} must divide heads and intermediate")
    hkv = cfg.kv_heads // tp if cfg.kv_heads >= tp else 1
    if cfg.kv_heads >= tp and cfg.kv_heads % tp:
        raise ValueError("tp must divide kv_heads (or exceed it)")
    vs = -(-cfg.vocab // tp)
    vs = (vs + 7) // 8 * 8
    return ShardDims(tp, rank, cfg.heads // tp, hkv, cfg.intermediate // tp, vs, rank * vs)


def _gen(seed: int, name: str, device) -> torch.Generator:
    h = int.from_bytes(hashlib.sha256(f"{seed}:{name}".encode()).digest()[:8], "little") & ((1 << 63) - 1)
    g = torch.Generator(device=device)
    g.manual_seed(h)
    return g


def _full(seed, name, shape, device, kind="normal"):
    g = _gen(seed, name, device)
    if kind == "norm":
        return 1.0 + 0.1 * torch.randn(*shape, generator=g, device=device)
    return torch.randn(*shape, generator=g, device=device) * 0.02


class RandomSource:
    """Deterministic random-init weights: every full tensor is generated from (seed, name), so
    any TP shard of it is identical to the same slice at tp=1."""

    def __init__(self, seed: int = 0, device="cpu"):
        self.seed, self.device = seed, device

    def region(self, name: str, shape, kind: str = "normal", rows: Optional[slice] = None,
               cols: Optional[slice] = None) -> torch.Tensor:
        t = _full(self.seed, name, shape, self.device, kind)
        if rows is not None:
            t = t[rows]
        if cols is not None:
            t = t[:, cols]
        return t


def hf_llama_name(name: str) -> str:
    """Canonical name (``l3.q``, ``embed``, ...) -> Hugging Face Llama safetensors key."""
    fixed = {"embed": "model.embed_tokens.weight", "lm_head": "lm_head.weight", "final_norm": "model.norm.weight"}
    if name in fixed:
        return fixed[name]
    layer, part = name[1:].split(".", 1)
    sub = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
           "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj",
           "attn_norm": "input_layernorm", "mlp_norm": "post_attention_layernorm"}[part]
    return f"model.layers.{layer}.{sub}.weight"


class CheckpointSource:
    """Weights from a safetensors file / shard directory, canonical or Hugging Face names.  Each
    TP rank reads only its slice of every matrix (memory-mapped region reads); a checkpoint
    without ``lm_head`` (tied embeddings) reuses ``embed``."""

    def __init__(self, path: str, device="cpu"):
        from ..utils.checkpoint import Checkpoint

        self.ck = Checkpoint(path)
        self.device = device

    def _key(self, name: str) -> str:
        from ..utils.checkpoint import CheckpointError

        for k in (name, hf_llama_name(name)):
            if k in self.ck:
                return k
        if name == "lm_head":
            return self._key("embed")
        raise CheckpointError(f"{self.ck.path}: no tensor for {name!r} (or {hf_llama_name(name)!r})")

    def region(self, name: str, shape, kind: str = "normal", rows: Optional[slice] = None,
               cols: Optional[slice] = None) -> torch.Tensor:
        from ..utils.checkpoint import CheckpointError

        key = self._key(name)
        have = self.ck.shape(key)
        if tuple(have) != tuple(shape):
            raise CheckpointError(f"{self.ck.path}: {key} has shape {tuple(have)}, config expects {tuple(shape)}")
        return self.ck.get_region(key, rows, cols).to(device=self.device, dtype=torch.float32)


def qkv_row_slices(cfg: LlamaConfig, tp: int, rank: int) -> Tuple[slice, slice]:
    """Rows of the full q and of the full k / v matrices that ``rank`` holds (a KV head is replicated over
    tp / kv_heads ranks when there are more ranks than KV heads)."""
    sd, D = shard_dims(cfg, tp, rank), cfg.head_dim
    kvh = (rank * cfg.kv_heads) // tp if cfg.kv_heads < tp else rank * sd.hkv
    return slice(rank * sd.hq * D, (rank + 1) * sd.hq * D), slice(kvh * D, (kvh + sd.hkv) * D)


LORA_TARGETS = {"q_proj": "q", "k_proj": "k", "v_proj": "v"}


def parse_lora_config(config: dict) -> Tuple[Tuple[str, ...], int, float, bool]:
    """``(modules, r, alpha, use_rslora)`` of a PEFT ``adapter_config.json`` dict (or the native form of
    the same keys); ``ValueError`` for everything the q/k/v LoRA path does not serve -- nothing is dropped."""
    targets = config.get("target_modules")
    if isinstance(targets, str) or not targets:
        raise ValueError(f"LoRA config: target_modules must be a list of module names, got {targets!r}")
    mods = []
    for t in targets:
        name = str(t).rsplit(".", 1)[-1]
        if name not in LORA_TARGETS and name not in LORA_TARGETS.values():
            raise ValueError(f"LoRA target module {t!r} is not served: only q_proj, k_proj and v_proj are")
        mods.append(LORA_TARGETS.get(name, name))
    if config.get("modules_to_save"):
        raise ValueError(f"LoRA config: modules_to_save {config['modules_to_save']!r} is not served")
    if config.get("bias", "none") not in ("none", None):
        raise ValueError(f"LoRA config: bias={config['bias']!r} is not served (bias terms)")
    if config.get("use_dora"):
        raise ValueError("LoRA config: DoRA (use_dora) is not served")
    for key in ("rank_pattern", "alpha_pattern"):
        if config.get(key):
            raise ValueError(f"LoRA config: {key} (per-layer ranks / alphas) is not served")
    if config.get("peft_type", "LORA") not in ("LORA", None):
        raise ValueError(f"LoRA config: peft_type {config['peft_type']!r} is not LoRA")
    r = config.get("r")
    if not isinstance(r, int) or not 1 <= r <= R.LORA_MAX_RANK:
        raise ValueError(f"LoRA config: rank r={r!r} outside 1..{R.LORA_MAX_RANK}")
    alpha = float(config.get("lora_alpha", r))
    return tuple(p for p in R.LORA_MODULES if p in mods), r, alpha, bool(config.get("use_rslora", False))


def random_lora_adapter(cfg: LlamaConfig, rank: int, seed: int = 0, modules=("q", "k", "v"), alpha: float = 32.0,
                        b_std: float = 0.02, device="cpu") -> Tuple[Dict[str, torch.Tensor], dict]:
    """A random adapter for tests and benchmarks, ``(tensors, config)`` for :meth:`LlamaTP.load_adapter`:
    drawn from :class:`RandomSource` under ``l{i}.{q,k,v}.lora_A/B``.  B is normal, not training's zero
    init: a zero delta would make every test of it vacuous."""
    src = RandomSource(seed, device)
    out = {"q": cfg.heads * cfg.head_dim, "k": cfg.kv_heads * cfg.head_dim, "v": cfg.kv_heads * cfg.head_dim}
    t: Dict[str, torch.Tensor] = {}
    for i in range(cfg.layers):
        for p in modules:
            t[f"l{i}.{p}.lora_A"] = src.region(f"l{i}.{p}.lora_A", (rank, cfg.hidden)) * (50.0 / cfg.hidden ** 0.5)
            t[f"l{i}.{p}.lora_B"] = src.region(f"l{i}.{p}.lora_B", (out[p], rank)) * (b_std / 0.02)
    return t, {"r": rank, "lora_alpha": alpha, "target_modules": [f"{p}_proj" for p in modules]}


def init_llama_shard(cfg: LlamaConfig, tp: int = 1, rank: int = 0, seed: int = 0, device="cpu",
                     dtype=torch.bfloat16, source=None) -> Dict[str, torch.Tensor]:
    """This rank's shard of a Llama: from ``source`` (:class:`CheckpointSource`) or a
    deterministic random init (:class:`RandomSource`, the same full model for every tp)."""
    src = source if source is not None else RandomSource(seed, device)
    sd = shard_dims(cfg, tp, rank)
    H, D = cfg.hidden, cfg.head_dim
    p: Dict[str, torch.Tensor] = {}

    def vocab_rows(name):
        lo, hi = sd.vocab_lo, min(cfg.vocab, sd.vocab_lo + sd.vocab_shard)
        out = torch.zeros(sd.vocab_shard, H, device=device)
        if hi > lo:
            out[: hi - lo] = src.region(name, (cfg.vocab, H), rows=slice(lo, hi)).to(device)
        return out.to(dtype)

    p["embed"] = vocab_rows("embed")
    p["lm_head"] = vocab_rows("lm_head")
    p["final_norm"] = src.region("final_norm", (H,), "norm").to(device=device, dtype=dtype)
    qs, ks = qkv_row_slices(cfg, tp, rank)
    sl = slice(rank * sd.inter, (rank + 1) * sd.inter)
    for i in range(cfg.layers):
        q = src.region(f"l{i}.q", (cfg.heads * D, H), rows=qs)
        k = src.region(f"l{i}.k", (cfg.kv_heads * D, H), rows=ks)
        v = src.region(f"l{i}.v", (cfg.kv_heads * D, H), rows=ks)
        p[f"l{i}.qkv"] = torch.cat([q, k, v]).to(device=device, dtype=dtype).contiguous()
        p[f"l{i}.o"] = src.region(f"l{i}.o", (H, cfg.heads * D), cols=qs).to(device=device, dtype=dtype).contiguous()
        p[f"l{i}.gate"] = src.region(f"l{i}.gate", (cfg.intermediate, H), rows=sl).to(device=device,
                                                                                      dtype=dtype).contiguous()
        p[f"l{i}.up"] = src.region(f"l{i}.up", (cfg.intermediate, H), rows=sl).to(device=device,
                                                                                  dtype=dtype).contiguous()
        p[f"l{i}.down"] = src.region(f"l{i}.down", (H, cfg.intermediate), cols=sl).to(device=device,
                                                                                      dtype=dtype).contiguous()
        p[f"l{i}.attn_norm"] = src.region(f"l{i}.attn_norm", (H,), "norm").to(device=device, dtype=dtype)
        p[f"l{i}.mlp_norm"] = src.region(f"l{i}.mlp_norm", (H,), "norm").to(device=device, dtype=dtype)
        del q, k, v
    return p


def full_llama_state(cfg: LlamaConfig, seed: int = 0, dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    """The unsharded random-init model under canonical names (what ``export-weights`` writes)."""
    src = RandomSource(seed)
    H, D = cfg.hidden, cfg.head_dim
    out = {"embed": src.region("embed", (cfg.vocab, H)), "lm_head": src.region("lm_head", (cfg.vocab, H)),
           "final_norm": src.region("final_norm", (H,), "norm")}
    for i in range(cfg.layers):
        for n, shp, kind in (("q", (cfg.heads * D, H), "normal"), ("k", (cfg.kv_heads * D, H), "normal"),
                             ("v", (cfg.kv_heads * D, H), "normal"), ("o", (H, cfg.heads * D), "normal"),
                             ("gate", (cfg.intermediate, H), "normal"), ("up", (cfg.intermediate, H), "normal"),
                             ("down", (H, cfg.intermediate), "normal"), ("attn_norm", (H,), "norm"),
                             ("mlp_norm", (H,), "norm")):
            out[f"l{i}.{n}"] = src.region(f"l{i}.{n}", shp, kind)
    return {k: v.to(dtype) for k, v in out.items()}


# --------------------------------------------------------------------------- tokenizer
class LlamaTokenizer:
    """Offline tokenizer: with a ``tokenizer.json`` the real BPE (``tokenizers``) is used;
    otherwise words are hashed into the vocab (synthetic ids) and decoded as ``<id>``."""

    _WORD = re.compile(r"\w+|[^\w\s]")

    def __init__(self, cfg: LlamaConfig, tokenizer_file: Optional[str] = None):
        self.cfg = cfg
        self._tok = None
        if tokenizer_file:
            from tokenizers import Tokenizer

            self._tok = Tokenizer.from_file(tokenizer_file)

    def encode(self, text: str) -> List[int]:
        if self._tok is not None:
            return [self.cfg.bos_id] + self._tok.encode(text).ids
        span = self.cfg.vocab - 1024
        return [self.cfg.bos_id] + [256 + zlib.crc32(w.encode()) % span for w in self._WORD.findall(text)]

    def decode(self, ids: Sequence[int]) -> str:
        if self._tok is not None:
            return self._tok.decode(list(ids))
        return " ".join(f"<{i}>" for i in ids)


# --------------------------------------------------------------------------- comm
class _ARDone:
    """A collective that already completed in stream order (or needed none)."""

    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        self.t = t

    def wait(self) -> torch.Tensor:
        return self.t


class _ARPending:
    """An all-reduce in flight on the backend's own stream (RCCL: ProcessGroupNCCL's NCCL stream,
    ordered after the producer on the current stream); :meth:`wait` orders the current stream
    after it -- the compute between start and wait overlaps the transfer."""

    __slots__ = ("t", "work")

    def __init__(self, t: torch.Tensor, work):
        self.t, self.work = t, work

    def wait(self) -> torch.Tensor:
        with tracing.range("tp.all_reduce_wait"):
            self.work.wait()
        return self.t


class TPComm:
    """Tensor-parallel collectives over a torch.distributed group (RCCL on GPU, gloo on CPU)."""

    def __init__(self, group=None, tp: int = 1, device=None, custom_ar: Optional[bool] = None):
        self.group = group
        self.tp = tp
        self.car = None
        if custom_ar is None:
            # on by default for TP > 1 on GPUs: a start-up self-test against the group's own
            # all-reduce gates it, and it is what lets the TP decode step run as one hipGraph
            custom_ar = os.environ.get("MLS_CUSTOM_AR", "1") == "1"
        if custom_ar and tp > 1 and device is not None and torch.device(device).type == "cuda":
            from ..parallel.custom_ar import CustomAllReduce

            car = CustomAllReduce(group, device)
            self.car = car if car.enabled else None
        # gloo with device tensors (TP rehearsal: several ranks sharing one GPU, where RCCL refuses
        # duplicate devices): stage the collectives through host memory
        self.host_staged = tp > 1 and dist.is_initialized() and dist.get_backend(group) == "gloo"

    def all_reduce_(self, t: torch.Tensor) -> torch.Tensor:
        if self.tp > 1:
            with tracing.range("tp.all_reduce"):
                return self._all_reduce(t)
        return t

    def _all_reduce(self, t: torch.Tensor) -> torch.Tensor:
        if self.car is not None and self.car.eligible(t):
            return self.car.all_reduce_(t)  # one-shot IPC path for small (decode) messages
        if self.host_staged and t.is_cuda:
            h = t.float().cpu()
            dist.all_reduce(h, group=self.group)
            t.copy_(h)
            return t
        dist.all_reduce(t, group=self.group)
        return t

    def all_reduce_start(self, t: torch.Tensor):
        """Start an in-place sum all-reduce and return a handle whose ``wait()`` yields ``t`` reduced.
        Large (prefill) messages go to the backend asynchronously so the caller can run independent
        work in between; the one-shot IPC path (an in-stream kernel) and host-staged gloo
        complete before returning."""
        if self.tp == 1:
            return _ARDone(t)
        with tracing.range("tp.all_reduce"):
            if (self.car is not None and self.car.eligible(t)) or (self.host_staged and t.is_cuda):
                return _ARDone(self._all_reduce(t))
            return _ARPending(t, dist.all_reduce(t, group=self.group, async_op=True))

    def all_gather(self, t: torch.Tensor) -> torch.Tensor:
        if self.tp == 1:
            return t.unsqueeze(0)
        with tracing.range("tp.all_gather"):
            return self._all_gather(t)

    def _all_gather(self, t: torch.Tensor) -> torch.Tensor:
        if self.host_staged and t.is_cuda:
            h = t.contiguous().cpu()
            out = [torch.empty_like(h) for _ in range(self.tp)]
            dist.all_gather(out, h, group=self.group)
            return torch.stack(out).to(t.device)
        out = [torch.empty_like(t) for _ in range(self.tp)]
        dist.all_gather(out, t.contiguous(), group=self.group)
        return torch.stack(out)

    def broadcast_(self, t: torch.Tensor, src: int = 0) -> torch.Tensor:
        if self.tp > 1:
            with tracing.range("tp.broadcast"):
                return self._broadcast(t, src)
        return t

    def _broadcast(self, t: torch.Tensor, src: int) -> torch.Tensor:
        if self.host_staged and t.is_cuda:
            h = t.cpu()
            dist.broadcast(h, src=src, group=self.group)
            t.copy_(h)
            return t
        dist.broadcast(t, src=src, group=self.group)
        return t


class ShardEmulationComm:
    """One TP rank's shard with every collective replaced by a local no-op -- a measurement tool:
    it times exactly the per-rank kernel work of a TP=tp decode / prefill step on one GPU (the
    all-reduce / all-gather cost is measured separately).  Outputs are not the model's."""

    graph_safe = True
    host_staged = False
    car = None

    def __init__(self, tp: int):
        self.tp = tp
        self.group = None

    def all_reduce_(self, t: torch.Tensor) -> torch.Tensor:
        return t

    def all_reduce_start(self, t: torch.Tensor):
        return _ARDone(t)

    def all_gather(self, t: torch.Tensor) -> torch.Tensor:
        return t.unsqueeze(0).expand(self.tp, *t.shape)

    def broadcast_(self, t: torch.Tensor, src: int = 0) -> torch.Tensor:
        return t


@dataclass
class GenParams:
    max_new_tokens: int = 16
    top_k: int = 1  # 1 = greedy
    temperature: float = 1.0
    seed: int = 0
    # LoRA adapter of the generation (LlamaTP.load_adapter's index; -1: the base model), or one per batch row
    adapter: Union[int, Sequence[int]] = -1


_M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sample_uniform(seed: int, step: int) -> float:
    """The sampling draw for (request seed, decode step): a counter-based hash, bit-identical to
    the device pick kernel (ops/csrc/decode_pick.hip), independent of the row's batch position."""
    h = _splitmix64(((int(seed) & _M64) * 0x9E3779B97F4A7C15 + int(step)) & _M64)
    return float(h >> 40) / 16777216.0


class TPCommError(RuntimeError):
    """A tensor-parallel collective lost a peer (one-shot all-reduce / all-gather timed out): the
    tokens of the affected generation are not trustworthy and the request fails."""


@dataclass
class _Forward:
    """What the pieces of one fused forward share: the step's route and inputs, and the residual
    stream as the layers advance it."""

    rt: StepRoute
    B: int
    S: int
    decode: bool
    pos: torch.Tensor  # [B * S] positions (clamped to the RoPE table)
    lens: torch.Tensor
    past: Optional[torch.Tensor]
    slots: Optional[torch.Tensor]  # prefill: explicit cache slot of every row (ops.prefill_slots)
    r: torch.Tensor  # residual stream (bf16)
    delta: Optional[torch.Tensor] = None  # the last row-parallel output, not yet added to r
    xn: Optional[torch.Tensor] = None  # RMSNorm(r) staged by _proj_add_norm for the next projection
    attn_kw: Optional[dict] = None  # LlamaTP._attention_kw
    # the layer tail's o-projection and gate_up outputs, held until the next layer's replace them: the
    # caching allocator then hands the next layer's temporaries other blocks than these, as it did when
    # the forward was one function whose locals lived that long.  Freed on return from the tail instead,
    # the captured batch-8 decode step measured 8 us (0.25 %) slower (docs/PERF_NOTES.md, "LlamaTP routing
    # refactor"; profiles/llama_route_keepalive_ab.jsonl)
    o: Optional[torch.Tensor] = None
    gu: Optional[torch.Tensor] = None
    lora_sid: Optional[torch.Tensor] = None  # cache slot of each sequence for the LoRA hook (None: the batch row)

    def take_xn(self) -> Optional[torch.Tensor]:
        xn, self.xn = self.xn, None
        return xn


class LlamaTP:
    """One rank of a tensor-parallel Llama with a KV cache ``[layers][max_batch, max_seq, hkv, D]``
    (or, paged, ``[layers][pages, 64, hkv, D]`` pools addressed through a page table)."""

    def __init__(self, params: Dict[str, torch.Tensor], cfg: LlamaConfig, tp: int = 1, rank: int = 0,
                 comm: Optional[TPComm] = None, backend: str = "reference", device="cpu", max_batch: int = 8,
                 max_seq: int = 1024, top_k_max: int = 50, kv_pages: int = 0, kv_dtype: str = "bf16",
                 weight_dtype: str = "bf16", kv_prefill: str = "rows", lora: Optional[dict] = None):
        """``lora={"max_adapters": n, "max_rank": r}``: room for n LoRA adapters of rank <= r on the q / k / v
        projections, chosen per cache slot (:meth:`load_adapter`, :meth:`set_slot_adapter`,
        ``GenParams.adapter``); until one is loaded neither backend computes anything new.
        ``kv_pages > 0``: paged KV cache -- per layer a pool of ``kv_pages`` pages of 64 rows
        shared by all sequences (:class:`~.kv_pages.PageTable`), instead of ``max_batch x max_seq``.
        ``kv_dtype="fp8"``: e4m3 KV rows with one fp32 scale per (row, KV head)
        (``ops.reference.kv_quant_fp8``) -- 132 instead of 256 bytes per head row.  Fused backend: uint8
        caches + scale tensors, written and read by ``ops.rope_kv_fp8_`` / ``ops.decode_attention_fp8``
        (head-major layout, head_dim 128, Hq / Hkv in 1, 2, 4, 8 only); reference backend: the fp32
        caches hold the round-tripped rows (the CPU oracle).  Prefill attention stays unquantised, unless
        ``kv_prefill="cache"`` (with ``kv_dtype="fp8"`` only; default ``"rows"``): every prefill attention
        then reads K / V from the cache, as decode does -- a forward appends its own rows first and reads
        them back quantised (reference: ``R.attention_ctx``, fused: ``ops.flash_attention_ctx_fp8``), the
        first chunk and a one-shot ``step(past=None)`` included, which run as ``past = 0``.  A token's
        logits then do not depend on how its prompt was chunked, on whether its prefix came from shared
        pages or on whether it was verified in a speculation step, so chunked prefill, prefix caching and
        speculative decoding are served with the e4m3 cache; prefill logits move from unquantised to e4m3
        rows.  The two-half TP-overlap prefill (``_prefill_overlapped``) attends the forward's own bf16
        rows, so it is not taken in this mode: the plain layer loop runs instead.
        ``weight_dtype="int4"``: W4A16 layer projections (qkv, o, gate / up, down) -- symmetric 4-bit
        codes with one bf16 scale per (row, 128 k) (``ops.reference.w4_quant``), quantised with the
        RMSNorm gains folded in; ``lm_head`` and the embedding stay bf16 (the usual quality choice).
        Both backends hold the dequantised product as the model's weights; the fused backend also
        keeps the packed codes (``self.w4``) and streams them in decode steps of up to
        ``w4_max_rows`` rows (``ops.skinny_w4``), larger steps run the bf16 rounding of the same
        weights.  Every quantised matrix needs K % 128 == 0 on this rank (row-parallel shards
        then cut K at group boundaries, so every TP degree sees the same groups).  Changes numerics.
        ``weight_dtype="w8a8"``: FP8 (e4m3) layer projections with e4m3 activations -- one fp32 scale per
        output channel (``ops.reference.w8_quant``, on the weights as held: gains folded, gate / up
        interleaved on the fused backend) and one dynamic scale per activation row
        (``ops.reference.a8_quant`` of the bf16-valued row that enters the projection; the two normalised
        projections quantise the un-normalised residual row and multiply its scale by its ``rstd``).
        ``lm_head`` and the embedding stay bf16.  One rule at every row count, so a row's result depends on
        that row alone and chunked prefill, prefix caching and speculation compose with it.  Reference
        backend: ``self.p`` holds the dequantised weights, ``self.w8`` the codes every projection multiplies
        (``ops.reference.w8a8_linear``).  Fused backend: ``self.w8`` holds ``ops.pack_w8``'s codes + scales
        and nothing else of a quantised matrix (no bf16, granule-packed or ``MLS_DECODE_FP8`` copy); every
        layer projection is ``ops.quant_rows_fp8`` + ``ops.gemm_w8a8`` (the block-scaled MFMA), the TP
        all-reduce and the split-KV combine run as their own launches.  Every layer matrix needs
        K % 128 == 0 and N % 16 == 0 on this rank (``ValueError`` otherwise: nothing falls back).  Changes
        numerics (e4m3 keeps 3 mantissa bits of weights AND activations); at TP > 1 a row-parallel projection
        quantises each rank's K slice with its own row scale, so logits differ slightly from TP = 1."""
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
        if weight_dtype not in ("bf16", "int4", "w8a8"):
            raise ValueError(f"weight_dtype must be 'bf16', 'int4' or 'w8a8', got {weight_dtype!r}")
        if kv_prefill not in ("rows", "cache"):
            raise ValueError(f"kv_prefill must be 'rows' or 'cache', got {kv_prefill!r}")
        if kv_prefill == "cache" and kv_dtype != "fp8":
            raise ValueError("kv_prefill='cache' is for kv_dtype='fp8' only: a bf16 cache already holds the very "
                             "rows prefill attends")
        self.kv_dtype = kv_dtype
        self.kv_prefill = kv_prefill
        self.weight_dtype = weight_dtype
        self.cfg = cfg
        self.sd = shard_dims(cfg, tp, rank)
        self.tp, self.rank = tp, rank
        self.comm = comm or TPComm(None, tp)
        # TP prefill as two interleaved batch halves (_prefill_overlapped); MLS_TP_OVERLAP=0: the plain layer loop
        self.tp_overlap = os.environ.get("MLS_TP_OVERLAP", "1") == "1"
        self.backend = backend
        self.device = torch.device(device)
        self.max_batch, self.max_seq = max_batch, max_seq
        self.top_k_max = top_k_max
        D = cfg.head_dim
        self.p = {k: v.to(self.device) for k, v in params.items()}
        # LoRA: adapter of every cache slot (-1: base), read in place by the captured steps
        self.lora_slot = torch.full((max_batch,), -1, dtype=torch.int32, device=self.device)
        self.lora_cfg = None if lora is None else {"max_adapters": int(lora.get("max_adapters", 8)),
                                                   "max_rank": int(lora.get("max_rank", 16))}
        self.lora_loaded: set = set()  # adapter indices in use
        self.lora_pack = None  # fused: ops.LoraPack
        self._lora_ref: List[Dict[int, dict]] = [dict() for _ in range(cfg.layers)]  # reference: layer -> index -> modules
        self._attn_gain: List[torch.Tensor] = []
        if self.lora_cfg is not None:
            if not 1 <= self.lora_cfg["max_rank"] <= R.LORA_MAX_RANK or self.lora_cfg["max_adapters"] < 1:
                raise ValueError(f"lora: max_rank must be in 1..{R.LORA_MAX_RANK} and max_adapters positive, "
                                 f"got {self.lora_cfg}")
            # the gains as given: both backends fold or overwrite them below
            self._attn_gain = [self.p[f"l{i}.attn_norm"].float().clone() for i in range(cfg.layers)]
        # int4: name -> (packed codes, scales) of the layer projections (fused backend only)
        self.w4: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.w4_max_rows = self.w4_variant = 0
        if weight_dtype == "int4":
            self._check_int4_shapes()
            if backend != "fused":
                self._quantise_reference()
        # w8a8: name -> (e4m3 codes, fp32 scales per output row, N); reference: codes [N, K], fused: ops.pack_w8's
        self.w8: Dict[str, Tuple[torch.Tensor, torch.Tensor, int]] = {}
        if weight_dtype == "w8a8":
            self._check_w8a8_shapes()
            if backend != "fused":
                self._quantise_reference_w8()
        # the fused forward's switches and copies of the weights (name -> tensors), set on both backends
        # so that whatever reads them needs no default; models/llama_route.py holds the rules they feed
        self.packed: Dict[str, torch.Tensor] = {}  # granule-packed bf16 copies (_pack_decode_copies)
        self.fp8: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}  # W8A8 e4m3 copies + scales
        self.pk_variant = int(os.environ.get("MLS_PACKED_VARIANT", "9"))
        self.pk_fold = os.environ.get("MLS_PACKED_FOLD", "1") == "1"  # residual adds in the o / down epilogues
        self.prefill_fold = os.environ.get("MLS_PREFILL_FOLD", "0") == "1"  # ... in prefill at TP = 1 too
        self.ar_fuse = os.environ.get("MLS_AR_FUSE", "1") == "1"  # GEMM-fused TP all-reduce (decode)
        self.ar_fused_calls = 0  # projections issued with the fused all-reduce (eager + captured)
        self.fuse_combine = os.environ.get("MLS_FUSE_COMBINE", "1") == "1"  # split-KV combine in the o prologue
        self.fuse_add_norm = True  # o / down through ops.linear_add_rmsnorm above 24 rows at TP = 1
        self.add_norm_fused = 0  # projections that took it
        self.dec_chunk = int(os.environ.get("MLS_DEC_CHUNK", "0"))  # decode split rows; 0: auto (llama_route)
        self.verify_attn = os.environ.get("MLS_VERIFY_ATTN", "multi")  # "ctx": verify through flash_attention_ctx
        if backend == "fused":
            from .. import ops

            self.ops = ops
            self._fold_and_quantise(weight_dtype)
            self._pack_decode_copies()
            self.ones = torch.ones(cfg.hidden, device=self.device, dtype=torch.bfloat16)
            self.workspace = torch.empty(32 << 20, device=self.device, dtype=torch.float32)
            self.dec_ws = torch.empty(max_batch * self.sd.hq * (-(-max_seq // 64)) * (D + 2) + 16,
                                      device=self.device, dtype=torch.float32)
            self.dec_cnt = torch.zeros(max_batch * self.sd.hkv, device=self.device, dtype=torch.int32)
            if self.lora_cfg is not None:
                self.lora_pack = ops.pack_lora(cfg.layers, cfg.hidden, tuple(h * D for h in (self.sd.hq, self.sd.hkv,
                                                                                             self.sd.hkv)),
                                               self.lora_cfg["max_adapters"], self.lora_cfg["max_rank"], self.device)
                # split-K slabs of every step up to 4096 rows (more rows run one split from a buffer of their own)
                self.lora_ws = torch.empty(self.lora_pack.workspace_elems(4096, 1), device=self.device,
                                           dtype=torch.float32)
            self.ver_ws: Optional[torch.Tensor] = None  # split-KV partials of the uncaptured verify steps
            self._ver_ws_graph: Optional[torch.Tensor] = None  # ... of the verify graph being warmed up / captured
        self._alloc_kv_cache(kv_pages)
        self.cos, self.sin = R.rope_tables(max_seq, D, cfg.rope_theta, self.device)
        # hipGraph capture of the decode step (P4): removes ~300 host launches per token.  With
        # tp > 1 the step's collectives are captured too: the one-shot IPC all-reduce is graph-safe
        # (device-side epochs), so with it enabled every decode batch whose messages it takes is
        # captured (see _graph_ok); RCCL collectives inside the graph are opt-in (MLS_TP_GRAPHS=1).
        self._rccl_graphs = (os.environ.get("MLS_TP_GRAPHS", "0") == "1"
                             and not getattr(self.comm, "host_staged", False))
        self.use_graphs = backend == "fused" and self.device.type == "cuda" and (
            tp == 1 or getattr(self.comm, "graph_safe", False) or self._rccl_graphs
            or getattr(self.comm, "car", None) is not None)
        self._graphs: Dict[Tuple[int, int, int], tuple] = {}
        self._ver_graphs: Dict[Tuple[int, int, int, int, str], tuple] = {}
        # speculative decoding: the most positions per sequence a verify step may carry (drafts + 1)
        self.spec_max_tokens = 8
        self.spec_stats = {"steps": 0, "drafted": 0, "accepted": 0}
        self._dec_ctx: Optional[int] = None  # host bound on decode context (sizes the split grid)
        # prefix caching (ContinuousLlama(prefix_cache=True) sets ctx_split): a prefill chunk of few
        # queries against a long cached context may run split-KV (ctx_splits); off: always one split
        self.ctx_split = False
        self.ctx_splits_forced = int(os.environ.get("MLS_CTX_SPLITS", "0"))  # A/B runs: this many splits
        self.ctx_ws: Optional[torch.Tensor] = None  # split-KV partials of the (uncaptured) prefill chunks
        # device-resident decode loop (X4 on device, _generate_device): per-batch-size static state
        # shared by the captured steps of every context bucket, so switching buckets copies nothing
        self._dev_graphs: Dict[Tuple[int, int, int], torch.cuda.CUDAGraph] = {}
        self._dev_state: Dict[int, Tuple[torch.Tensor, ...]] = {}
        self._serve: Dict[int, Dict[str, torch.Tensor]] = {}
        self.keep_logits = False
        self.last_logits: Optional[torch.Tensor] = None
        self.health_every = int(os.environ.get("MLS_TP_HEALTH_EVERY", "32"))

    def _check_int4_shapes(self) -> None:
        cfg, fused = self.cfg, self.backend == "fused"
        for i in range(cfg.layers):
            for n in ("qkv", "o", "gate", "up", "down"):
                N_, K_ = self.p[f"l{i}.{n}"].shape
                if K_ % R.W4_GROUP or (fused and N_ % (8 if n in ("gate", "up") else 16)):
                    raise ValueError(f"weight_dtype='int4': l{i}.{n} is [{N_}, {K_}] on this rank (tp {self.tp}); "
                                     f"needs K % {R.W4_GROUP} == 0" + (", N % 16 == 0" if fused else ""))

    def _quantise_reference(self) -> None:
        """``weight_dtype="int4"`` on the reference backend, the CPU oracle: gains folded as ops.fold_norm
        (fp32 product, one bf16 rounding), then the exact dequantised product as the weights; the folded
        norms become ones."""
        for i in range(self.cfg.layers):
            for n, gain in (("qkv", "attn_norm"), ("gate", "mlp_norm"), ("up", "mlp_norm"), ("o", None), ("down", None)):
                w = self.p[f"l{i}.{n}"]
                if gain is not None:
                    w = (w.float() * self.p[f"l{i}.{gain}"].float().view(1, -1)).to(w.dtype)
                self.p[f"l{i}.{n}"] = R.w4_dequant(*R.w4_quant(w))
            for gain in ("attn_norm", "mlp_norm"):
                self.p[f"l{i}.{gain}"] = torch.ones_like(self.p[f"l{i}.{gain}"])

    def _check_w8a8_shapes(self) -> None:
        for i in range(self.cfg.layers):
            for n in ("qkv", "o", "gate", "up", "down"):
                N_, K_ = self.p[f"l{i}.{n}"].shape
                if K_ % 128 or N_ % 16:
                    raise ValueError(f"weight_dtype='w8a8': l{i}.{n} is [{N_}, {K_}] on this rank (tp {self.tp}); "
                                     f"needs K % 128 == 0 and N % 16 == 0")

    def _quantise_reference_w8(self) -> None:
        """``weight_dtype="w8a8"`` on the reference backend, the CPU oracle: gains folded as ops.fold_norm,
        then ``R.w8_quant``: ``self.w8`` keeps the codes + scales the projections multiply, ``self.p`` the
        exact dequantised product under the unchanged keys; the folded norms become ones."""
        for i in range(self.cfg.layers):
            for n, gain in (("qkv", "attn_norm"), ("gate", "mlp_norm"), ("up", "mlp_norm"), ("o", None), ("down", None)):
                w = self.p[f"l{i}.{n}"]
                if gain is not None:
                    w = (w.float() * self.p[f"l{i}.{gain}"].float().view(1, -1)).to(w.dtype)
                q, sc = R.w8_quant(w)
                self.w8[f"l{i}.{n}"] = (q, sc, w.shape[0])
                self.p[f"l{i}.{n}"] = R.w8_dequant(q, sc)
            for gain in ("attn_norm", "mlp_norm"):
                self.p[f"l{i}.{gain}"] = torch.ones_like(self.p[f"l{i}.{gain}"])

    def _alloc_kv_cache(self, kv_pages: int) -> None:
        """The per-layer K / V caches (paged pools with ``kv_pages > 0``), their layout flags and, for an
        e4m3 cache on the fused backend, the scale tensors."""
        cfg, sd, D = self.cfg, self.sd, self.cfg.head_dim
        max_batch, max_seq, fused = self.max_batch, self.max_seq, self.backend == "fused"
        cdt = torch.bfloat16 if fused else torch.float32
        # fused: head-major caches ([.., Hkv, rows, D]) -- one head's rows contiguous, so a decode split
        # block streams one 16 KiB run instead of 64 slices of 256 B (MLS_KV_HEAD_MAJOR=0: row-major)
        self.kv_hm = fused and os.environ.get("MLS_KV_HEAD_MAJOR", "1") == "1"
        self.pages = None
        if kv_pages > 0:
            from .kv_pages import PageTable

            self.page_rows = 64  # = the decode split: one page per split block
            self.pages = PageTable(kv_pages, self.page_rows, max_batch, -(-max_seq // self.page_rows), self.device)
            shape = (kv_pages, sd.hkv, self.page_rows, D) if self.kv_hm else (kv_pages, self.page_rows, sd.hkv, D)
        else:
            shape = (max_batch, sd.hkv, max_seq, D) if self.kv_hm else (max_batch, max_seq, sd.hkv, D)
        self.kv_hm_rows = 0 if not self.kv_hm else (self.page_rows if kv_pages > 0 else max_seq)
        self.kv_fp8 = fused and self.kv_dtype == "fp8"
        self.k_scale: List[torch.Tensor] = []
        self.v_scale: List[torch.Tensor] = []
        if self.kv_fp8:
            # the matrix-core decode kernel's own limits; no fallback to bf16 rows
            G = sd.hq // max(sd.hkv, 1)
            bad = [why for ok, why in (
                (self.kv_hm, "the head-major cache layout (MLS_KV_HEAD_MAJOR=0 is set)"),
                (D == 128, f"head_dim 128 (got {D})"),
                (sd.hq % sd.hkv == 0 and G in (1, 2, 4, 8), f"Hq / Hkv in 1, 2, 4, 8 (got {sd.hq} / {sd.hkv})"),
                (self.dec_chunk in (0, 64, 128), f"decode splits of 64 or 128 rows (MLS_DEC_CHUNK={self.dec_chunk})"),
                (kv_pages > 0 or max_seq % 4 == 0, f"max_seq a multiple of 4 (got {max_seq})"),
            ) if not ok]
            if bad:
                raise ValueError("kv_dtype='fp8' on the fused backend needs " + "; ".join(bad))
            cdt = torch.uint8
            self.k_scale = [torch.zeros(shape[:3], device=self.device, dtype=torch.float32) for _ in range(cfg.layers)]
            self.v_scale = [torch.zeros_like(self.k_scale[0]) for _ in range(cfg.layers)]
        self.k_cache = [torch.zeros(shape, device=self.device, dtype=cdt) for _ in range(cfg.layers)]
        self.v_cache = [torch.zeros_like(self.k_cache[0]) for _ in range(cfg.layers)]

    def _fold_and_quantise(self, weight_dtype: str) -> None:
        """The fused backend's weights as its kernels read them: gate / up interleaved, the RMSNorm gains
        folded into the projections that consume the normalised activations, and with
        ``weight_dtype="int4"`` the layer projections quantised as held then."""
        ops, cfg = self.ops, self.cfg
        for i in range(cfg.layers):
            gu = ops.interleave_gate_up(self.p.pop(f"l{i}.gate"), self.p.pop(f"l{i}.up"))
            mlp_g = self.p.pop(f"l{i}.mlp_norm")
            self.p[f"l{i}.gate_up"] = ops.fold_norm(gu, mlp_g)
            self.p[f"l{i}.qkv"] = ops.fold_norm(self.p[f"l{i}.qkv"], self.p.pop(f"l{i}.attn_norm"))
        self.p["lm_head"] = ops.fold_norm(self.p["lm_head"], self.p.pop("final_norm"))
        if weight_dtype == "w8a8":
            # quantised as held here; the codes + scales are ALL the model keeps of a layer matrix
            for i in range(cfg.layers):
                for n in ("qkv", "o", "gate_up", "down"):
                    w = self.p.pop(f"l{i}.{n}")
                    self.w8[f"l{i}.{n}"] = (*ops.pack_w8(w), w.shape[0])
                    del w
        if weight_dtype != "int4":
            return
        # quantised as held here (gain folded, gate / up interleaved: a row permutation).  p
        # keeps the bf16 rounding of the dequantised matrix for the > w4_max_rows GEMMs
        # (prefill, chunked prefill), w4 the packed codes the decode steps stream; no
        # granule-packed bf16 copy of these names (_pack_decode_copies)
        for i in range(cfg.layers):
            for n in ("qkv", "o", "gate_up", "down"):
                q, sc = R.w4_quant(self.p[f"l{i}.{n}"])
                self.p[f"l{i}.{n}"] = R.w4_dequant(q, sc).to(torch.bfloat16)
                self.w4[f"l{i}.{n}"] = ops.pack_skinny_w4_codes(q, sc)
                del q, sc
        # decode steps up to this many rows stream the int4 codes: the kernel's own limit (the
        # measurements behind it: llama_route.proj_tiers)
        self.w4_max_rows = min(32, int(os.environ.get("MLS_W4_MAX_ROWS", "32")))
        self.w4_variant = int(os.environ.get("MLS_W4_VARIANT", "0"))  # probe knob: the launch shape

    def _pack_decode_copies(self) -> None:
        """The second copies of the projections that decode-shaped steps stream (``self.packed``,
        ``self.fp8``); a matrix held as int4 codes gets neither."""
        ops, cfg = self.ops, self.cfg
        if self.device.type != "cuda":
            return
        names = [f"l{i}.{n}" for i in range(cfg.layers) for n in ("qkv", "o", "gate_up", "down")] + ["lm_head"]
        names = [n for n in names if n in self.p]  # w8a8: the layer matrices live in self.w8 alone
        # Decode (<= 24 tokens per step) streams a second, granule-packed copy of every projection
        # (ops.pack_skinny: each wave reads contiguous 1 KiB granules, non-temporal): 3.4-4.5 ->
        # 4.6-6.2 TB/s on the Llama-3-8B shapes (profiles/r2_decode_packed_weight_probe.jsonl).
        # Costs one more copy of the weights in HBM (16 GB at 8B / TP = 1 of 288 GB);
        # MLS_PACKED_DECODE=0 turns it off, "auto" packs while the copy stays under 1/4 of the card.
        mode = os.environ.get("MLS_PACKED_DECODE", "auto")
        if mode != "0":
            fit = [n for n in names if self.p[n].shape[0] % 16 == 0 and self.p[n].shape[1] % 32 == 0
                   and self.p[n].numel() * 2 < (1 << 31) and n not in self.w4]
            total = sum(self.p[n].numel() * 2 for n in fit)
            cap = torch.cuda.get_device_properties(self.device).total_memory
            if mode == "1" or total <= cap // 4:
                self.packed = {n: ops.pack_skinny(self.p[n]) for n in fit}
        # Opt-in FP8 decode (MLS_DECODE_FP8=1): W8A8 e4m3 copies of the projections, per-channel
        # weight scales and per-row activation scales (ops.skinny_fp8), for <= 4 tokens per step --
        # half the weight stream (profiles/r2_decode_fp8_weight_probe.jsonl).  Changes numerics
        # (e4m3 has a 3-bit mantissa), so bf16 stays the default.
        if os.environ.get("MLS_DECODE_FP8", "0") == "1":
            # only matrices of >= 16M weights: below that a decode GEMM is latency-bound and the
            # fp8 prologue (row |max| reduction + requantisation) costs more than the bytes saved
            # -- one emulated TP = 8 rank was 1.13 -> 1.18 ms/token with every projection in fp8
            min_el = int(os.environ.get("MLS_DECODE_FP8_MIN", str(1 << 24)))
            self.fp8 = {n: ops.pack_skinny_fp8(self.p[n]) for n in names
                        if self.p[n].shape[0] % 16 == 0 and self.p[n].shape[1] % 64 == 0
                        and min_el <= self.p[n].numel() < (1 << 31) and n not in self.w4}  # int4 wins

    # ---------------------------------------------------------------- shared pieces
    @property
    def qkv_width(self) -> int:
        return (self.sd.hq + 2 * self.sd.hkv) * self.cfg.head_dim

    def layer_weight_bytes(self) -> int:
        """Bytes of the layer projections a decode step streams on this rank: the int4 codes + scales
        where the model holds them (fused ``weight_dtype="int4"``), the e4m3 codes + scales of fused
        ``weight_dtype="w8a8"``, else the matrices as held."""
        total = 0
        if self.backend == "fused":
            total += sum(t.numel() * t.element_size() for wq, ws, _ in self.w8.values() for t in (wq, ws))
        for name, w in self.p.items():
            if name.rsplit(".", 1)[-1] in ("qkv", "o", "gate", "up", "gate_up", "down"):
                held = self.w4.get(name, (w,))
                total += sum(t.numel() * t.element_size() for t in held)
        return total

    def _embed(self, ids: torch.Tensor) -> torch.Tensor:
        sd = self.sd
        if self.backend == "fused":
            x = self.ops.embedding(ids, self.p["embed"], lo=sd.vocab_lo, hi=sd.vocab_lo + sd.vocab_shard)
        else:
            local = ids.long() - sd.vocab_lo
            ok = (local >= 0) & (local < sd.vocab_shard)
            x = self.p["embed"][local.clamp(0, sd.vocab_shard - 1)].float() * ok.unsqueeze(-1)
        return self.comm.all_reduce_(x)

    def _local_topk(self, logits: torch.Tensor, k: int):
        if self.keep_logits:  # tests: the full (shard-local) last-token logits of the latest step
            self.last_logits = logits
        if self.backend == "fused":  # shard offset + padded-tail mask inside the merge launch
            return self.ops.topk_large(logits, k, lo=self.sd.vocab_lo, valid=self.cfg.vocab - self.sd.vocab_lo)
        else:
            vals, idx = torch.topk(logits.float(), k, dim=-1)
            idx = idx.to(torch.int32)
        # mask rows of the padded vocab tail
        idx = idx + self.sd.vocab_lo
        vals = torch.where(idx < self.cfg.vocab, vals, torch.full_like(vals, float("-inf")))
        return vals, idx

    def _merge_sample(self, vals: torch.Tensor, idx: torch.Tensor, gp: GenParams, step: int) -> torch.Tensor:
        """X4: all-gather the ranks' top-k candidates, merge, pick the next token (identical on
        every rank: same inputs, same counter-based draw -> no broadcast needed)."""
        cv, ci = self.gather_candidates(vals, idx)
        return torch.tensor([self.pick_token(cv[b], ci[b], gp, step) for b in range(cv.shape[0])],
                            dtype=torch.int32, device=vals.device)

    # ---------------------------------------------------------------- reference backend
    def _ref_layer(self, i: int, x: torch.Tensor, B: int, S: int, positions: torch.Tensor, lens: torch.Tensor,
                   slots_b: torch.Tensor, decode: bool, past: Optional[torch.Tensor] = None) -> torch.Tensor:
        cfg, sd, p = self.cfg, self.sd, self.p
        D = cfg.head_dim
        w8 = self.weight_dtype == "w8a8"
        if w8:
            qkv = self._ref_w8(f"l{i}.qkv", x, norm=True)
        else:
            xn = R.layernorm(x, p[f"l{i}.attn_norm"], None, eps=cfg.eps, rms=True)[0]
            qkv = xn @ p[f"l{i}.qkv"].float().T
        if self.lora_loaded:
            qkv = R.lora_qkv(qkv, x, self._attn_gain[i], self._lora_ref[i], self.lora_slot, B, S,
                             (sd.hq * D, sd.hkv * D, sd.hkv * D), slot_ids=slots_b, eps=cfg.eps)
        T = qkv.shape[0]
        # chunked prefill: a padding row's position may lie past the RoPE table (it is never stored)
        rpos = positions if past is None else positions.clamp(max=self.max_seq - 1)
        q = R.rope(qkv[:, : sd.hq * D].view(T, sd.hq, D), rpos, self.cos, self.sin)
        k = R.rope(qkv[:, sd.hq * D: (sd.hq + sd.hkv) * D].view(T, sd.hkv, D), rpos, self.cos, self.sin)
        v = qkv[:, (sd.hq + sd.hkv) * D:].view(T, sd.hkv, D)
        b_of = torch.arange(B, device=x.device).repeat_interleave(T // B)
        valid = positions < self.max_seq
        if not decode:
            valid = valid & (positions < lens.long()[b_of])
        rows = b_of if slots_b is None else slots_b.long()[b_of]  # batch row -> cache row
        bi, pi = rows[valid], positions[valid].long()
        k_st, v_st = k[valid], v[valid]
        # the cache holds what an e4m3 row + scale gives back (kv_prefill="rows": prefill stays unquantised;
        # "cache": every prefill comes with past and attends these rows below)
        if self.kv_dtype == "fp8":
            k_st = R.kv_dequant_fp8(*R.kv_quant_fp8(k_st))
            v_st = R.kv_dequant_fp8(*R.kv_quant_fp8(v_st))
        if self.pages is not None:  # paged: flat pool rows through the page table
            flat = self.pages.rows(bi, pi)
            self.k_cache[i].view(-1, sd.hkv, D)[flat] = k_st.to(self.k_cache[i].dtype)
            self.v_cache[i].view(-1, sd.hkv, D)[flat] = v_st.to(self.v_cache[i].dtype)
        else:
            self.k_cache[i][bi, pi] = k_st.to(self.k_cache[i].dtype)
            self.v_cache[i][bi, pi] = v_st.to(self.v_cache[i].dtype)
        if decode:
            qrow = q.reshape(B, sd.hq * D)
            if self.pages is not None:  # gather each sequence's pages back into [B, rows, hkv, D]
                table = self.pages.device_table()[:B].long()
                kv = [c[table].reshape(B, -1, sd.hkv, D) for c in (self.k_cache[i], self.v_cache[i])]
                a = R.decode_attention(qrow, kv[0], kv[1], lens, sd.hq, sd.hkv, D)
            else:
                a = R.decode_attention(qrow, self.k_cache[i][:B], self.v_cache[i][:B], lens, sd.hq, sd.hkv, D)
        else:
            qkv_r = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], dim=1)
            if past is not None:  # chunked prefill: the chunk attends to the cache rows just written
                table = self.pages.device_table() if self.pages is not None else None
                a = R.attention_ctx(qkv_r, self.k_cache[i], self.v_cache[i], past, lens, B, S, sd.hq, sd.hkv, D,
                                    slot_ids=slots_b, page_table=table)
            else:
                a = R.attention(qkv_r, B, S, sd.hq, sd.hkv, D, kv_lens=lens, causal=True)
        if w8:
            x = x + self.comm.all_reduce_(self._ref_w8(f"l{i}.o", a))
            h = F.silu(self._ref_w8(f"l{i}.gate", x, norm=True)) * self._ref_w8(f"l{i}.up", x, norm=True)
            return x + self.comm.all_reduce_(self._ref_w8(f"l{i}.down", h))
        o = self.comm.all_reduce_(a @ p[f"l{i}.o"].float().T)
        x = x + o
        xn = R.layernorm(x, p[f"l{i}.mlp_norm"], None, eps=cfg.eps, rms=True)[0]
        h = F.silu(xn @ p[f"l{i}.gate"].float().T) * (xn @ p[f"l{i}.up"].float().T)
        d = self.comm.all_reduce_(h @ p[f"l{i}.down"].float().T)
        return x + d

    def _ref_w8(self, name: str, x: torch.Tensor, norm: bool = False) -> torch.Tensor:
        """The W8A8 projection of the rows ``x`` (rounded to bf16) by W_name; ``norm``: of RMSNorm(x), its gain
        folded into W -- the un-normalised row is quantised and rstd multiplies its scale."""
        h = x.to(torch.bfloat16)
        rstd = torch.rsqrt(h.float().pow(2).mean(-1) + self.cfg.eps) if norm else None
        wq, ws, _ = self.w8[name]
        return R.w8a8_linear(h, wq, ws, rstd)

    def _ref_forward(self, ids: torch.Tensor, positions: torch.Tensor, lens: torch.Tensor, B: int, S: int,
                     decode: bool, k: int, slot_ids: Optional[torch.Tensor] = None,
                     past: Optional[torch.Tensor] = None, all_rows: bool = False):
        x = self._embed(ids.reshape(-1))
        for i in range(self.cfg.layers):
            x = self._ref_layer(i, x, B, S, positions.reshape(-1), lens, slot_ids, decode, past)
        xn = R.layernorm(x, self.p["final_norm"], None, eps=self.cfg.eps, rms=True)[0]
        if not decode and not all_rows:
            n = lens.long() if past is None else lens.long() - past.long()  # valid rows of this forward
            last = (torch.arange(B, device=x.device) * S + n - 1)
            xn = xn[last]
        logits = xn @ self.p["lm_head"].float().T
        return self._local_topk(logits, k)

    # ---------------------------------------------------------------- fused backend
    def _route(self, B: int, S: int, decode: bool, has_past: bool, all_rows: bool) -> StepRoute:
        """The kernels this forward runs (models/llama_route.py), from host values alone: nothing here
        reads a device tensor, so it is safe inside graph capture."""
        sd, cfg = self.sd, self.cfg
        car = getattr(self.comm, "car", None) if self.tp > 1 else None  # both questions below arise at TP > 1 only
        return step_route(
            B=B, S=S, decode=decode, has_past=has_past, all_rows=all_rows, tp=self.tp, hq=sd.hq, hkv=sd.hkv,
            head_dim=cfg.head_dim, hidden=cfg.hidden, have_packed=bool(self.packed), have_w4=bool(self.w4),
            have_w8=bool(self.w8),
            have_fp8=bool(self.fp8), o_packed="l0.o" in self.packed, o_fp8="l0.o" in self.fp8, kv_fp8=self.kv_fp8,
            w4_max_rows=self.w4_max_rows, pk_fold=self.pk_fold, prefill_fold=self.prefill_fold,
            fuse_combine=self.fuse_combine, fuse_add_norm=self.fuse_add_norm, ar_fuse=self.ar_fuse,
            tp_overlap=self.tp_overlap and not self.lora_loaded, verify_attn=self.verify_attn,
            spec_max_tokens=self.spec_max_tokens,
            dec_chunk=self.dec_chunk, ar_fusable=car is not None and car.fusable(B * S * cfg.hidden),
            capturing=self.tp > 1 and self.device.type == "cuda" and torch.cuda.is_current_stream_capturing())

    # -- projections: one walk down the ladder of weight copies (llama_route.ProjTiers)
    def _skinny(self, tr: ProjTiers, name: str, K: int):
        """The decode kernel over the copy of W_name that ``tr``'s row count streams -- int4 codes, e4m3,
        granule-packed bf16, in that order -- as ``f(x, **kw)``; None: the model holds no such copy (or
        the rows are too many), the caller runs the row-major matrix.  A w8a8 matrix has one route at every
        row count: quantise the rows, then the block-scaled MFMA GEMM."""
        ops = self.ops
        if name in self.w8:
            if not tr.w8:
                raise RuntimeError(f"{name} is held as w8a8 codes only, and the route has no w8a8 tier")
            return self._w8_proj(name)
        N = self.p[name].shape[0]
        if tr.w4 and name in self.w4:
            return lambda x, **kw: ops.skinny_w4(x, *self.w4[name], N, variant=self.w4_variant, **kw)
        if tr.fp8_for(K) and name in self.fp8:
            return lambda x, **kw: ops.skinny_fp8(x, *self.fp8[name], N, **kw)
        if tr.packed and name in self.packed:
            return lambda x, **kw: ops.skinny_packed(x, self.packed[name], N, variant=self.pk_variant, **kw)
        return None

    def _w8_proj(self, name: str):
        ops, (wq, ws, N) = self.ops, self.w8[name]

        def run(x, delta=None, resid_out=None, norm=False, act=ops.ACT_NONE, eps=1e-5, residual=None):
            xq, xs = ops.quant_rows_fp8(x, delta, resid_out, norm=norm, eps=eps)
            return ops.gemm_w8a8(xq, xs, wq, ws, N, act=act, residual=residual, workspace=self.workspace)

        return run

    def _proj(self, tr: ProjTiers, x: torch.Tensor, name: str, residual: Optional[torch.Tensor] = None):
        """``x @ W_name^T (+ residual)``."""
        skinny = self._skinny(tr, name, x.shape[1])
        if skinny is not None:
            return skinny(x, residual=residual)
        return self.ops.linear(x, self.p[name], residual=residual, workspace=self.workspace)

    def _norm_proj(self, tr: ProjTiers, x: torch.Tensor, name: str, d: Optional[torch.Tensor] = None,
                   act=None, xn: Optional[torch.Tensor] = None, resid_out: bool = True, impl: str = "auto"):
        """``(act(RMSNorm(x + d) @ W_name^T), residual)`` with the gain folded into W.  The residual
        stream after the add is ``x`` itself without ``d``, else a new tensor (the one-launch kernels)
        or ``x`` updated in place (RMSNorm + GEMM) -- unless ``resid_out`` is off: then ``x + d`` is
        written nowhere.  ``xn``: RMSNorm(x) as a preceding :meth:`_proj_add_norm` staged it (``d`` is
        None then); ``impl``: ``ops.linear``'s, above 16 rows."""
        ops, eps, ws = self.ops, self.cfg.eps, self.workspace
        w = self.p.get(name)  # None: held as w8a8 codes, which _skinny routes below
        act = ops.ACT_NONE if act is None else act
        if xn is not None:
            return ops.linear(xn, w, act=act, workspace=ws), x
        skinny = self._skinny(tr, name, x.shape[1])
        if skinny is None and not tr.fuse:
            if d is None:
                xn = ops.rmsnorm(x, self.ones, eps=eps)
            else:
                xn = ops.rmsnorm(d, self.ones, residual=x, residual_out=x if resid_out else None, eps=eps)
            return ops.linear(xn, w, act=act, workspace=ws, impl=impl), x
        r_new = torch.empty_like(x) if d is not None and resid_out else None
        if skinny is not None:
            y = skinny(x, delta=d, resid_out=r_new, norm=True, act=act, eps=eps)
        else:
            y = ops.gemm_rmsnorm(x, w, d, r_new, act=act, eps=eps, workspace=ws)
        return y, (x if r_new is None else r_new)

    def _row_parallel(self, rt: StepRoute, x: torch.Tensor, name: str) -> torch.Tensor:
        """sum over the TP ranks of x @ W_name^T (W row-parallel: each rank holds a K slice)."""
        if rt.ar_fuse and name in self.packed and not (rt.proj.fp8_for(x.shape[1]) and name in self.fp8):
            self.ar_fused_calls += 1
            with tracing.range("tp.gemm_all_reduce"):
                return self.ops.skinny_packed_ar(x, self.packed[name], self.p[name].shape[0], self.comm.car,
                                                 variant=self.pk_variant)
        return self.comm.all_reduce_(self._proj(rt.proj, x, name))

    def _proj_add_norm(self, x: torch.Tensor, name: str, r: torch.Tensor) -> Optional[torch.Tensor]:
        """``r += x @ W_name^T`` in place and RMSNorm(r) for the next projection
        (``ops.linear_add_rmsnorm``); None, with nothing launched, where that op has no route."""
        xn = self.ops.linear_add_rmsnorm(x, self.p[name], r, self.ones, self.cfg.eps, self.workspace)
        if xn is not None:
            self.add_norm_fused += 1
        return xn

    # -- attention
    def _verify_workspace(self, T: int, chunk: int) -> torch.Tensor:
        """Split-KV partials of a verify step (``ops.decode_attention_multi``) of T rows."""
        sd, D = self.sd, self.cfg.head_dim
        cap = self.pages.pages_per_seq * self.page_rows if self.pages is not None else self.max_seq
        return self._verify_ws(T * sd.hq * (-(-min(self._dec_ctx or cap, cap) // chunk)) * (D + 2))

    def _verify_ws(self, need: int) -> torch.Tensor:
        """``need`` fp32 elements of split-KV partials for a verify step, captured or not."""
        # a captured step owns its workspace (_verify_graph keeps it alive with the graph, whose launches
        # hold its address); only the uncaptured steps share one, which may therefore be regrown
        ws = self._ver_ws_graph
        if ws is None:
            if self.ver_ws is None or self.ver_ws.numel() < need:
                self.ver_ws = torch.empty(need, device=self.device, dtype=torch.float32)
            ws = self.ver_ws
        elif ws.numel() < need:
            ws = self._ver_ws_graph = torch.empty(need, device=self.device, dtype=torch.float32)
        return ws

    def _ctx_split_kw(self, B: int, S: int, max_ctx: Optional[int], verify: bool = False) -> dict:
        """Prefix caching on: a prefill chunk of few queries against a long cached context runs split-KV
        where :meth:`ctx_splits` says so.  ``verify``: a verify step on the context kernel (the e4m3
        cache) -- the same rule under the step's own context bound, its partials in the verify
        workspace (a captured step's graph owns it)."""
        sd, D = self.sd, self.cfg.head_dim
        cap = self.pages.pages_per_seq * self.page_rows if self.pages is not None else self.max_seq
        ctx_max = min(int(max_ctx) if max_ctx else cap, cap)  # no host bound given: what a slot holds
        n_split = self.ctx_splits(B, S, sd.hq, ctx_max)
        if n_split <= 1:
            return {}
        need = self.ops.flash_ctx_workspace_elems(B, S, sd.hq, D, n_split)
        if verify:
            return dict(splits=n_split, max_ctx=ctx_max, workspace=self._verify_ws(need))
        if self.ctx_ws is None or self.ctx_ws.numel() < need:
            self.ctx_ws = torch.empty(need, device=self.device, dtype=torch.float32)
        return dict(splits=n_split, max_ctx=ctx_max, workspace=self.ctx_ws)

    def _attention_kw(self, rt: StepRoute, B: int, S: int, decode: bool, pos: torch.Tensor, sid, past, all_rows: bool,
                      max_ctx: Optional[int]) -> dict:
        """What every layer's attention call of one step has in common, built once."""
        table = self.pages.dev if self.pages is not None else None
        if decode:  # RoPE + KV append ride inside the decode-attention launch
            kw = dict(workspace=self.dec_ws, counters=self.dec_cnt, positions=pos, cos=self.cos, sin=self.sin,
                      max_len=self._dec_ctx, combine=not rt.fuse_combine,
                      chunk=rt.dec_chunk if table is None else self.page_rows,
                      page_table=None if table is None else table[:B])
            if not self.kv_fp8:
                kw["head_major"] = self.kv_hm
            return kw
        if rt.multi:
            chunk = self.page_rows if table is not None else (rt.dec_chunk if rt.dec_chunk in (64, 128) else 64)
            return dict(slot_ids=sid, chunk=chunk, max_len=self._dec_ctx, page_table=table,
                        workspace=self._verify_workspace(B * S, chunk))
        if past is not None:  # chunked prefill: the chunk's queries against the cache rows just written
            if all_rows and self.kv_fp8:  # a verify step, <= 8 queries against the whole context: always routed
                split = self._ctx_split_kw(B, S, self._dec_ctx, verify=True)
            else:
                split = self._ctx_split_kw(B, S, max_ctx) if self.ctx_split and not all_rows else {}
            return dict(slot_ids=sid, page_table=table, **split)
        return {}

    def _rope_kv(self, i: int, qkv: torch.Tensor, pos, slots, lens, S: int, flat_off: Optional[int] = None) -> None:
        """RoPE on the Q / K heads of ``qkv`` in place + the append of its K / V rows to layer i's cache
        (an e4m3 cache: quantised; qkv keeps the unquantised bf16 K / V that kv_prefill="rows" attends).
        ``flat_off``: the bf16 caches from that element on, flattened (implicit slots of a batch half)."""
        sd = self.sd
        args = (qkv, pos, self.cos, self.sin, sd.hq, sd.hkv, self.cfg.head_dim, slots)
        kw = dict(lens=lens, seq=S, max_seq=self.max_seq, hm_rows=self.kv_hm_rows)
        if self.kv_fp8:
            self.ops.rope_kv_fp8_(*args, self.k_cache[i], self.v_cache[i], self.k_scale[i], self.v_scale[i], **kw)
        elif flat_off is None:
            self.ops.rope_kv_(*args, self.k_cache[i], self.v_cache[i], **kw)
        else:
            self.ops.rope_kv_(*args, self.k_cache[i].reshape(-1)[flat_off:], self.v_cache[i].reshape(-1)[flat_off:], **kw)

    def _fused_attention(self, i: int, qkv: torch.Tensor, st: "_Forward"):
        """Layer i's attention for the step's ``qkv`` rows, RoPE and the KV append included: ``(a, parts)``,
        ``parts`` the split-KV partials where their combine rides in the o-projection, else None."""
        ops, sd, D = self.ops, self.sd, self.cfg.head_dim
        kc, vc = self.k_cache[i], self.v_cache[i]
        if st.decode:
            caches = (kc, vc, self.k_scale[i], self.v_scale[i]) if self.kv_fp8 else (kc, vc)  # e4m3: same partials
            if self.pages is None:
                caches = [c[:st.B] for c in caches]
            attend = ops.decode_attention_fp8 if self.kv_fp8 else ops.decode_attention
            a = attend(qkv, *caches, st.lens, sd.hq, sd.hkv, D, **st.attn_kw)
            return a if st.rt.fuse_combine else (a, None)
        self._rope_kv(i, qkv, st.pos, st.slots, st.lens, st.S)
        if st.rt.multi:
            return ops.decode_attention_multi(qkv, kc, vc, st.past, st.lens, st.B, st.S, sd.hq, sd.hkv, D,
                                              **st.attn_kw), None
        if st.past is not None and self.kv_fp8:
            return ops.flash_attention_ctx_fp8(qkv, kc, vc, self.k_scale[i], self.v_scale[i], st.past, st.lens, st.B,
                                               st.S, sd.hq, sd.hkv, D, **st.attn_kw), None
        if st.past is not None:
            return ops.flash_attention_ctx(qkv, kc, vc, st.past, st.lens, st.B, st.S, sd.hq, sd.hkv, D,
                                           **st.attn_kw), None
        return ops.flash_attention(qkv, st.B, st.S, sd.hq, sd.hkv, D, kv_lens=st.lens, causal=True), None

    # -- after attention: o-projection -> gate_up -> down, in the shape the route names
    def _layer_tail(self, i: int, st: "_Forward", a: torch.Tensor, parts) -> None:
        rt = st.rt
        if rt.fold:
            self._tail_folded(i, st, a, parts)
            return
        # o (and, if it can, down) through ops.linear_add_rmsnorm; where o_proj has no such route, or an
        # earlier layer left a delta, the all-reduce pair
        staged = rt.fuse_rn and st.delta is None and self._tail_staged(i, st, a)
        if not staged:
            self._tail_reduced(i, st, a, parts)

    def _o_combine(self, rt: StepRoute, name: str, a: torch.Tensor, parts, residual=None) -> torch.Tensor:
        """The o-projection with the split-KV combine in its prologue (one launch, not two) and, at
        TP > 1 where it can, the all-reduce in its epilogue; otherwise this rank's partial sum."""
        N = self.p[name].shape[0]
        if rt.ar_fuse:
            self.ar_fused_calls += 1
            with tracing.range("tp.gemm_all_reduce"):
                return self.ops.skinny_packed_combine_ar(a, parts, self.packed[name], N, self.comm.car,
                                                         variant=self.pk_variant)
        return self.ops.skinny_packed_combine(a, parts, self.packed[name], N, residual=residual, variant=self.pk_variant)

    def _tail_folded(self, i: int, st: "_Forward", a: torch.Tensor, parts) -> None:
        """TP = 1: h = r + a Wo^T, r' = h + g Wd^T, both adds in the GEMM epilogues; no delta."""
        tr = st.rt.proj
        if parts is not None:
            h = self._o_combine(st.rt, f"l{i}.o", a, parts, residual=st.r)
        else:
            h = self._proj(tr, a, f"l{i}.o", residual=st.r)
        st.o = h
        gu, _ = self._norm_proj(tr, h, f"l{i}.gate_up", act=self.ops.ACT_SILU_MUL)
        st.gu = gu
        st.r = self._proj(tr, gu, f"l{i}.down", residual=h)

    def _tail_staged(self, i: int, st: "_Forward", a: torch.Tensor) -> bool:
        """o_proj, and down_proj where it can (never the last layer's: the lm_head reads r and delta),
        add into r in place and stage RMSNorm(r) for the next projection.  False, with nothing
        launched, if o_proj has no such route."""
        xn = self._proj_add_norm(a, f"l{i}.o", st.r)
        if xn is None:
            return False
        gu, st.r = self._norm_proj(st.rt.proj, st.r, f"l{i}.gate_up", act=self.ops.ACT_SILU_MUL, xn=xn)
        st.gu = gu
        if i + 1 < self.cfg.layers:
            st.xn = self._proj_add_norm(gu, f"l{i}.down", st.r)  # delta stays None: the down output is in r
        if st.xn is None:
            st.delta = self._row_parallel(st.rt, gu, f"l{i}.down")
        return True

    def _tail_reduced(self, i: int, st: "_Forward", a: torch.Tensor, parts) -> None:
        """The all-reduce pair: o and down each summed over the ranks, each added to r by the pre-norm
        of the projection after it (delta)."""
        rt = st.rt
        if parts is None:
            o = self._row_parallel(rt, a, f"l{i}.o")
        else:
            o = self._o_combine(rt, f"l{i}.o", a, parts)
            if not rt.ar_fuse:
                o = self.comm.all_reduce_(o)
        st.o = o
        gu, st.r = self._norm_proj(rt.proj, st.r, f"l{i}.gate_up", o, act=self.ops.ACT_SILU_MUL)
        st.gu = gu
        st.delta = self._row_parallel(rt, gu, f"l{i}.down")

    def _fused_forward(self, ids: torch.Tensor, positions: torch.Tensor, lens: torch.Tensor, B: int, S: int,
                       decode: bool, k: int, slot_ids: Optional[torch.Tensor] = None,
                       past: Optional[torch.Tensor] = None, all_rows: bool = False, max_ctx: Optional[int] = None):
        """Native-kernel forward.  The RMSNorm gains are folded into the following projections, so
        for decode-shaped token counts (<= 16) each pre-norm + residual add rides inside the skinny
        GEMM (``ops.gemm_rmsnorm``: 7 launches per layer); larger counts run a gain-free RMSNorm and
        the library / native GEMM (``ops.linear``).  Which kernels: :meth:`_route`."""
        ops, cfg = self.ops, self.cfg
        rt = self._route(B, S, decode, past is not None, all_rows)
        pos = positions.reshape(-1)
        slots = sid = None
        if (slot_ids is not None or self.pages is not None or past is not None) and not decode:
            # prefill into arbitrary cache rows (continuous batching) / through the page table: one
            # native launch (ops.prefill_slots), -1 past each sequence's length
            sid = None if slot_ids is None else slot_ids.to(torch.int32)
            if self.pages is not None:
                slots = ops.prefill_slots(pos, lens, B, S, sid, table=self.pages.device_table(),
                                          page_rows=self.pages.page_rows)
            else:
                slots = ops.prefill_slots(pos, lens, B, S, sid, max_seq=self.max_seq)
        if past is not None:  # a padding row's position may lie past the RoPE table (its slot is -1 already)
            pos = pos.clamp(max=self.max_seq - 1)
        st = _Forward(rt, B, S, decode, pos, lens, past, slots, r=self._embed(ids.reshape(-1)))
        if self.lora_loaded and slot_ids is not None and not decode:
            st.lora_sid = slot_ids.to(torch.int32)
        if rt.overlap:
            st.r, st.delta = self._prefill_overlapped(rt, st.r, pos, lens, B, S, slots)
        else:
            st.attn_kw = self._attention_kw(rt, B, S, decode, pos, sid, past, all_rows, max_ctx)
            for i in range(cfg.layers):
                qkv, st.r = self._norm_proj(rt.proj, st.r, f"l{i}.qkv", st.delta, xn=st.take_xn())
                if self.lora_loaded:
                    self._lora_fused(i, qkv, st)
                a, parts = self._fused_attention(i, qkv, st)
                self._layer_tail(i, st, a, parts)
        r, delta = st.r, st.delta
        if not decode and not all_rows:  # each sequence's last valid token (one native gather of r and delta)
            rows = lens if past is None else lens - past  # valid rows of this forward (on the device)
            if delta is None:
                r = ops.last_rows(r, rows, B, S)
            else:
                r, delta = ops.last_rows(r, rows, B, S, delta)
        # the lm_head down the same ladder at its own row count (B, or every row of the step with all_rows):
        # never int4; r + delta is not written back; above 16 rows -- 1 GB of weights -- the weight-streaming
        # native tile up to 64 rows, the tile GEMM above (delta is None there when the residual adds rode
        # in the o / down epilogues: int4 steps of 25-32 rows)
        nb = r.shape[0]
        head = proj_tiers(nb, bool(self.packed), False, bool(self.fp8), 0)
        logits, _ = self._norm_proj(head, r, "lm_head", delta, resid_out=False, impl="native" if nb <= 64 else "auto")
        return self._local_topk(logits, k)

    def _prefill_overlapped(self, rt: StepRoute, r, pos, lens, B: int, S: int, explicit_slots):
        """TP prefill as two batch halves (micro-batches) interleaved layer by layer so that every
        o / down all-reduce runs while the other half computes:

            half 0: norm+QKV, RoPE/KV, attention, o -> start AR(o0)
            half 1: norm+QKV, RoPE/KV, attention, o -> start AR(o1)     [overlaps AR(o0)]
            half 0: wait AR(o0), norm+gate/up, down -> start AR(d0)     [overlaps AR(o1)]
            half 1: wait AR(o1), norm+gate/up, down -> start AR(d1)     [overlaps AR(d0)]
            next layer, half 0 waits AR(d0)                             [overlaps AR(d1)]

        The residual stream rows of each half are updated in place (views of ``r``); returns the
        full residual and the last layer's all-reduced delta."""
        ops, cfg, sd, tr = self.ops, self.cfg, self.sd, rt.proj
        D = cfg.head_dim
        half = B // 2
        # plain cache: each half runs rope_kv_'s implicit slot mode (token t -> row (t // S) * max_seq
        # + pos) on a view of the caches starting at its first batch row -- no torch-side slot map
        # (the head-major layout groups hm_rows slots, so the offset must be a whole group)
        # (the fp8 cache takes explicit slots: its scale tensors would need a second offset view)
        implicit = (explicit_slots is None and not self.kv_fp8
                    and (not self.kv_hm_rows or (half * self.max_seq) % self.kv_hm_rows == 0))
        if explicit_slots is None and not implicit:
            explicit_slots = ops.prefill_slots(pos, lens, B, S, max_seq=self.max_seq)
        slot_elems = sd.hkv * D  # cache elements per slot in either layout
        parts = [(0, half), (half, B)]
        res = [r[b0 * S:b1 * S] for b0, b1 in parts]
        dlt = [None, None]
        pend_d = [None, None]
        for i in range(cfg.layers):
            pend_o = [None, None]
            for m, (b0, b1) in enumerate(parts):
                lo, hi = b0 * S, b1 * S
                if pend_d[m] is not None:
                    dlt[m] = pend_d[m].wait()
                qkv, res[m] = self._norm_proj(tr, res[m], f"l{i}.qkv", dlt[m])
                if implicit:
                    self._rope_kv(i, qkv, pos[lo:hi], None, lens[b0:b1], S, flat_off=b0 * self.max_seq * slot_elems)
                else:
                    self._rope_kv(i, qkv, pos[lo:hi], explicit_slots[lo:hi], lens[b0:b1], S)
                a = ops.flash_attention(qkv, b1 - b0, S, sd.hq, sd.hkv, D, kv_lens=lens[b0:b1], causal=True)
                pend_o[m] = self.comm.all_reduce_start(self._proj(tr, a, f"l{i}.o"))
            for m in range(2):
                o = pend_o[m].wait()
                gu, res[m] = self._norm_proj(tr, res[m], f"l{i}.gate_up", o, act=ops.ACT_SILU_MUL)
                pend_d[m] = self.comm.all_reduce_start(self._proj(tr, gu, f"l{i}.down"))
        dlt = [p.wait() for p in pend_d]
        if any(x.data_ptr() != y.data_ptr() for x, y in zip(res, (r[:half * S], r[half * S:]))):
            r = torch.cat(res)  # _norm_proj handed back new residual tensors instead of the views
        return r, torch.cat(dlt)

    # ---------------------------------------------------------------- LoRA adapters (q / k / v)
    def _lora_fused(self, i: int, qkv: torch.Tensor, st: "_Forward") -> None:
        """``qkv += s B (A . RMSNorm(st.r))`` in place for the rows whose slot names an adapter
        (``ops.lora_qkv_``: two launches, device arrays only)."""
        ops, pack, rows = self.ops, self.lora_pack, st.B * st.S
        nsplit = ops.lora_split(st.B, st.S, self.cfg.hidden, pack.rcap)
        ws = self.lora_ws
        if pack.workspace_elems(rows, nsplit) > ws.numel():
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"LoRA: a captured step of {rows} rows exceeds the model's split-K workspace")
            ws = torch.empty(pack.workspace_elems(rows, nsplit), device=self.device, dtype=torch.float32)
        ops.lora_qkv_(qkv, st.r, pack, i, self.lora_slot, st.B, st.S, st.lora_sid, eps=self.cfg.eps, workspace=ws,
                      nsplit=nsplit)

    def load_adapter(self, index: int, tensors: Dict[str, torch.Tensor], config: dict) -> None:
        """Load LoRA adapter ``index`` in place (fixed addresses: steps captured with an adapter loaded stay
        valid; the first load drops the steps captured before it, which hold no LoRA launches).  ``tensors``:
        the unsharded ``l{i}.{q,k,v}.lora_A [r, hidden]`` / ``.lora_B [out, r]`` of every layer; ``config``:
        PEFT's keys (``r``, ``lora_alpha``, ``use_rslora``, ``target_modules``).  Each rank keeps A whole and
        the rows of B that it holds of the base matrices.  ``ValueError`` for whatever is not served
        (:func:`parse_lora_config`), a bad index, shapes that disagree with the config."""
        if self.lora_cfg is None:
            raise ValueError("this model was built without lora=...: no room for adapters")
        if not isinstance(index, int) or not 0 <= index < self.lora_cfg["max_adapters"]:
            raise ValueError(f"adapter index {index!r} outside [0, {self.lora_cfg['max_adapters']}): more adapters "
                             f"than max_adapters")
        mods, r, alpha, rslora = parse_lora_config(config)
        if r > self.lora_cfg["max_rank"]:
            raise ValueError(f"adapter rank {r} exceeds the model's lora max_rank {self.lora_cfg['max_rank']}")
        cfg, D = self.cfg, self.cfg.head_dim
        qs, ks = qkv_row_slices(cfg, self.tp, self.rank)
        full = {"q": cfg.heads * D, "k": cfg.kv_heads * D, "v": cfg.kv_heads * D}
        local: Dict[str, torch.Tensor] = {}
        for i in range(cfg.layers):
            for p in mods:
                try:
                    A, Bm = tensors[f"l{i}.{p}.lora_A"], tensors[f"l{i}.{p}.lora_B"]
                except KeyError as e:
                    raise ValueError(f"adapter has no tensor {e.args[0]!r} (target module {p}_proj)") from None
                if tuple(A.shape) != (r, cfg.hidden) or tuple(Bm.shape) != (full[p], r):
                    raise ValueError(f"l{i}.{p}: lora_A {tuple(A.shape)} / lora_B {tuple(Bm.shape)} do not match the "
                                     f"config: expected ({r}, {cfg.hidden}) / ({full[p]}, {r})")
                local[f"l{i}.{p}.lora_A"] = A
                local[f"l{i}.{p}.lora_B"] = Bm[qs if p == "q" else ks]
        extra = [k for k in tensors if k not in local]
        if extra:
            raise ValueError(f"adapter tensors outside the config's target modules: {sorted(extra)[:4]}")
        scales = {p: R.lora_scale(alpha, r, rslora) for p in mods}
        if self.backend == "fused":
            self.lora_pack.load(index, local, scales, gains=self._attn_gain)
        else:
            for i in range(cfg.layers):
                self._lora_ref[i][index] = {p: (local[f"l{i}.{p}.lora_A"].to(self.device, torch.float32),
                                                local[f"l{i}.{p}.lora_B"].to(self.device, torch.float32), scales[p])
                                            for p in mods}
        if not self.lora_loaded:
            # steps captured so far hold no LoRA launches (nothing new runs while no adapter is loaded): drop
            # them, the next step captures again with the hook in.  Later loads rewrite fixed addresses only.
            self._graphs.clear()
            self._ver_graphs.clear()
            self._dev_graphs.clear()
        self.lora_loaded.add(index)

    def set_slot_adapter(self, slot: int, index: int) -> None:
        """Cache slot ``slot`` serves adapter ``index`` (-1: the base model) from the next step on."""
        if not isinstance(slot, int) or not 0 <= slot < self.max_batch:
            raise ValueError(f"slot {slot!r} outside [0, {self.max_batch})")
        if not isinstance(index, int) or (index != -1 and index not in self.lora_loaded):
            raise ValueError(f"adapter {index!r} is not loaded (loaded: {sorted(self.lora_loaded)}; -1 = base)")
        self.lora_slot[slot] = index

    def set_batch_adapters(self, B: int, adapter: Union[int, Sequence[int]]) -> None:
        """Slots 0 .. B - 1 (the rows of a ``generate`` batch) take ``adapter``: one index, or one per row."""
        idx = [int(adapter)] * B if isinstance(adapter, int) else [int(a) for a in adapter]
        if len(idx) != B:
            raise ValueError(f"{len(idx)} adapter indices for a batch of {B}")
        if B > self.max_batch:
            raise ValueError("batch exceeds the KV cache")
        for a in idx:
            if a != -1 and a not in self.lora_loaded:
                raise ValueError(f"adapter {a!r} is not loaded (loaded: {sorted(self.lora_loaded)}; -1 = base)")
        self.lora_slot[:B] = torch.tensor(idx, dtype=torch.int32).to(self.device)

    # ---------------------------------------------------------------- public
    def check_prefill_chunk(self) -> None:
        """Chunked prefill (``step(past=...)``) reads its context from the KV cache: raises
        ``ValueError`` for the configurations it does not serve (nothing falls back to one shot)."""
        if self.kv_dtype == "fp8" and self.kv_prefill != "cache":
            raise ValueError("chunked prefill is not available with kv_dtype='fp8': one-shot prefill attends the "
                             "unquantised rows, a chunk reading e4m3 context would change the numerics")
        if self.backend == "fused":
            if not self.kv_hm:
                raise ValueError("chunked prefill on the fused backend needs the head-major KV cache "
                                 "(MLS_KV_HEAD_MAJOR=0 is set)")
            if self.cfg.head_dim != 128:
                raise ValueError(f"chunked prefill on the fused backend needs head_dim 128 (got {self.cfg.head_dim})")

    def check_speculate(self, speculate: int = 1) -> None:
        """Speculative decoding (``verify_step`` of ``speculate + 1`` positions per sequence) reads its
        context from the KV cache like a prefill chunk: raises ``ValueError`` for what that refuses and,
        on the fused backend, for more positions x query heads per KV head than the verify attention's
        16 lane columns (nothing falls back to the chunk kernel)."""
        speculate = int(speculate)
        if speculate < 1 or speculate + 1 > self.spec_max_tokens:
            raise ValueError(f"speculate must be in [1, {self.spec_max_tokens - 1}], got {speculate}")
        try:
            self.check_prefill_chunk()
        except ValueError as e:
            raise ValueError(str(e).replace("chunked prefill", "speculative decoding")) from None
        if self.backend == "fused":
            G = self.sd.hq // max(self.sd.hkv, 1)
            if G not in (1, 2, 4, 8) or (speculate + 1) * G > 16:
                raise ValueError(f"speculative decoding on the fused backend needs Hq / Hkv in 1, 2, 4, 8 and "
                                 f"(speculate + 1) * Hq / Hkv <= 16 (got speculate {speculate}, "
                                 f"{self.sd.hq} / {self.sd.hkv} heads on this rank)")

    def check_prefix_cache(self) -> None:
        """Prefix caching shares filled KV pages between sequences and prefills a suffix against them
        like a prefill chunk: raises ``ValueError`` without the paged cache and for what chunked
        prefill refuses (nothing falls back to recomputing the prefix)."""
        if self.pages is None:
            raise ValueError("prefix caching needs the paged KV cache (kv_pages is 0): it shares pages, "
                             "a per-slot cache has none")
        try:
            self.check_prefill_chunk()
        except ValueError as e:
            raise ValueError(str(e).replace("chunked prefill", "prefix caching")) from None

    # split-KV routing of a prefill chunk (ops.flash_attention_ctx(splits=...)).  The constants come from
    # the kernel table of docs/PERF_NOTES.md "Prefix caching" (profiles/prefix_cache_ab.jsonl; Hq 32, Hkv 8,
    # paged, unsplit -> routed, us): 32 blocks x 65 tiles 112 -> 25 (16 splits), 128 blocks x 68 tiles
    # 117 -> 45 (4), 256 blocks x 65 tiles 118 -> 85 (2; 4 splits 94), 1024 blocks x 20 tiles 84 -> 92 (2
    # splits lose).  One tile per split loses to two and four (32 blocks x 17 tiles: 16.7 / 13.8 / 14.2).
    CTX_SPLIT_BLOCKS = 512     # bring the grid to this many blocks; at or above it: unsplit
    CTX_SPLIT_MIN_TILES = 4    # every split keeps at least this many 64-key tiles
    CTX_SPLIT_MAX = 16         # the largest count measured

    @classmethod
    def ctx_split_rule(cls, B: int, S: int, Hq: int, max_ctx: Optional[int]) -> int:
        """Splits of a prefill chunk's context attention: a host-side function of the launch shape and
        the host bound on ``past + n`` alone.  The largest power of two (the counts measured) that is
        at most ``CTX_SPLIT_BLOCKS`` / the unsplit grid's blocks, leaves every split
        ``CTX_SPLIT_MIN_TILES`` key tiles and does not exceed ``CTX_SPLIT_MAX``; 1 otherwise."""
        if max_ctx is None:
            return 1
        blocks = -(-S // 64) * Hq * B
        tiles = -(-int(max_ctx) // 64)
        n = min(-(-cls.CTX_SPLIT_BLOCKS // blocks), tiles // cls.CTX_SPLIT_MIN_TILES, cls.CTX_SPLIT_MAX)
        return 1 << (n.bit_length() - 1) if n >= 2 else 1

    def ctx_splits(self, B: int, S: int, Hq: int, max_ctx: Optional[int]) -> int:
        """:meth:`ctx_split_rule`, unless ``MLS_CTX_SPLITS=n`` forces n (A/B runs)."""
        if self.ctx_splits_forced > 0:
            return max(1, min(64, self.ctx_splits_forced))
        return self.ctx_split_rule(B, S, Hq, max_ctx)

    def _verify_graph(self, B: int, T: int, k: int, ctx: int):
        """Captured verify step for B sequences of T positions under the context bound ctx (static id /
        past / lens / slot buffers, as :meth:`_decode_graph`).  Warm-up and capture run with
        ``lens == past``: every row is padding, so no cache row is written."""
        key = (B, T, k, ctx, self.verify_attn)  # one graph per attention route (A/B arms)
        if key in self._ver_graphs:
            return self._ver_graphs[key]
        dev = self.device
        ids = torch.zeros(B, T, dtype=torch.int32, device=dev)
        past = torch.zeros(B, dtype=torch.int32, device=dev)
        lens = torch.zeros(B, dtype=torch.int32, device=dev)
        slots = torch.arange(B, dtype=torch.int32, device=dev)
        off = torch.arange(T, dtype=torch.int32, device=dev).unsqueeze(0)
        if self.pages is not None:
            self.pages.device_table()

        def run():
            return self.step(ids, past.unsqueeze(1) + off, lens, decode=False, k=k, slot_ids=slots, past=past,
                             all_rows=True)

        # this graph's own split-KV workspace: the first warm-up step sizes it, the capture bakes its address
        self._ver_ws_graph = torch.empty(0, device=dev, dtype=torch.float32)
        try:
            g, (vals, idx) = self._capture(ctx, run, run)
        finally:
            ws, self._ver_ws_graph = self._ver_ws_graph, None
        # off and ws stay referenced: the captured launches read / write them at every replay
        self._ver_graphs[key] = (g, ids, past, lens, slots, vals, idx, off, ws)
        return self._ver_graphs[key]

    @torch.no_grad()
    def verify_step(self, ids: torch.Tensor, past: torch.Tensor, n: torch.Tensor, k: int,
                    slot_ids: Optional[torch.Tensor] = None, max_ctx: Optional[int] = None):
        """Speculative decoding's one forward: row b feeds ``n[b] <= T`` tokens ``ids[b, :n[b]]`` at
        positions ``past[b] ..`` of cache slot ``slot_ids[b]`` (default b) and gets the local top-k of
        every position, ``(vals, idx) [B, T, k]``.  Rows ``t >= n[b]`` are padding: never stored, their
        candidates unspecified.  ``max_ctx``: a host bound on ``past + n`` (sizes the split grid).  On
        the fused backend the step is a graph replay per (B, T, k, context bucket)."""
        B, T = ids.shape
        dev = self.device
        self.check_speculate(max(1, T - 1))
        ids = ids.to(dev).to(torch.int32)
        past = past.to(dev).to(torch.int32).view(B)
        lens = past + n.to(dev).to(torch.int32).view(B)
        slots = (torch.arange(B, dtype=torch.int32, device=dev) if slot_ids is None
                 else slot_ids.to(dev).to(torch.int32).view(B))
        ctx = self.ctx_bucket(max_ctx)
        if self.use_graphs and self._graph_ok(B * T):
            g, i_s, p_s, l_s, s_s, v_s, x_s = self._verify_graph(B, T, k, ctx)[:7]
            if self.pages is not None:
                self.pages.device_table()  # the graph reads the table buffer in place
            i_s.copy_(ids)
            p_s.copy_(past)
            l_s.copy_(lens)
            s_s.copy_(slots)
            with tracing.range("llama.verify"):
                g.replay()
            return v_s.view(B, T, -1), x_s.view(B, T, -1)
        pos = past.unsqueeze(1) + torch.arange(T, dtype=torch.int32, device=dev).unsqueeze(0)
        self._dec_ctx = ctx if self.backend == "fused" else None
        try:
            vals, idx = self.step(ids, pos, lens, decode=False, k=k, slot_ids=slots, past=past, all_rows=True)
        finally:
            self._dec_ctx = None
        return vals.view(B, T, -1), idx.view(B, T, -1)

    @torch.no_grad()
    def step(self, ids: torch.Tensor, positions: torch.Tensor, lens: torch.Tensor, decode: bool, k: int,
             slot_ids: Optional[torch.Tensor] = None, past: Optional[torch.Tensor] = None, all_rows: bool = False,
             max_ctx: Optional[int] = None):
        """One forward.  ``max_ctx`` (with ``past``): a host bound on ``lens`` -- with prefix caching on
        it decides whether the chunk's attention runs split-KV (:meth:`ctx_splits`) and where the
        splits are cut.  ``slot_ids`` (prefill only): cache row of each batch row (default: the
        batch row itself) -- how continuous batching prefills new requests into free slots.
        ``past`` (prefill only, int32 ``[B]``): rows of each sequence already in the cache -- this
        forward is the chunk at ``positions`` ``past[b] + i`` (absolute), ``lens`` the absolute end
        after it; its attention reads the cache (``ops.flash_attention_ctx``) and the returned
        candidates are those of row ``lens[b] - past[b] - 1``.
        ``all_rows`` (with ``past``): the candidates of EVERY row, ``[B*S, k]`` -- a speculative-decoding
        verify step (:meth:`verify_step`); rows at or past ``lens[b] - past[b]`` are padding."""
        B, S = ids.shape
        if all_rows and past is None:
            raise ValueError("all_rows needs past (a verify step reads its context from the cache)")
        ids, positions, lens = ids.contiguous(), positions.contiguous(), lens.contiguous()
        if past is None and not decode and self.kv_prefill == "cache":
            past = torch.zeros(B, dtype=torch.int32, device=self.device)  # one shot = the chunk at past 0
        if past is not None:
            if decode:
                raise ValueError("past is a prefill argument")
            self.check_prefill_chunk()
            past = past.to(self.device).to(torch.int32).contiguous()
        if self.pages is not None and not (self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            self.pages.device_table()
        if slot_ids is not None:
            slot_ids = slot_ids.to(self.device).contiguous()
        with tracing.range("llama.decode" if decode else "llama.prefill"):
            if self.backend == "fused":
                return self._fused_forward(ids.to(torch.int32), positions.to(torch.int32), lens.to(torch.int32), B,
                                           S, decode, k, slot_ids, past, all_rows, max_ctx)
            return self._ref_forward(ids, positions, lens, B, S, decode, k, slot_ids, past, all_rows)

    @torch.no_grad()
    def prefill_chunked(self, ids: torch.Tensor, lens: torch.Tensor, chunk: int, k: int,
                        slot_ids: Optional[torch.Tensor] = None):
        """Prefill the prompt batch ``ids [B, S]`` (right-padded, ``lens [B]``) in chunks of ``chunk``
        positions: chunk c is one ``step(past=c * chunk)`` over the rows whose prompt has not ended
        (the others drop out), as wide as the longest of them needs.  Returns ``(vals, idx)``
        ``[B, k]`` -- each row's candidates from the chunk that holds its last prompt token."""
        chunk = int(chunk)
        if chunk <= 0:
            raise ValueError(f"chunk must be positive, got {chunk}")
        self.check_prefill_chunk()
        B, S = ids.shape
        dev = self.device
        lens_h = [int(x) for x in lens.detach().to("cpu").tolist()]
        if len(lens_h) != B or min(lens_h) < 1 or max(lens_h) > min(S, self.max_seq):
            raise ValueError(f"lens must be in [1, {min(S, self.max_seq)}] for each of the {B} sequences")
        ids = ids.to(dev)
        vals = idx = None
        for s0 in range(0, max(lens_h), chunk):
            rows = [b for b in range(B) if lens_h[b] > s0]
            w = min(chunk, max(lens_h[b] for b in rows) - s0)
            rt = torch.tensor(rows, dtype=torch.long, device=dev)
            ends = torch.tensor([min(lens_h[b], s0 + w) for b in rows], dtype=torch.int32, device=dev)
            past = torch.full((len(rows),), s0, dtype=torch.int32, device=dev)
            pos = (s0 + torch.arange(w, dtype=torch.int32, device=dev)).unsqueeze(0).expand(len(rows), w).contiguous()
            sid = rt.to(torch.int32) if slot_ids is None else slot_ids.to(dev)[rt].to(torch.int32)
            v, i = self.step(ids[rt, s0: s0 + w], pos, ends, decode=False, k=k, slot_ids=sid, past=past)
            if vals is None:
                vals = torch.zeros((B, *v.shape[1:]), dtype=v.dtype, device=v.device)
                idx = torch.zeros((B, *i.shape[1:]), dtype=i.dtype, device=i.device)
            fin = [j for j, b in enumerate(rows) if lens_h[b] <= s0 + w]  # rows whose prompt ends in this chunk
            if fin:
                src = torch.tensor(fin, dtype=torch.long, device=v.device)
                dst = torch.tensor([rows[j] for j in fin], dtype=torch.long, device=v.device)
                vals[dst] = v[src]
                idx[dst] = i[src]
        return vals, idx

    def _prefill(self, ids: torch.Tensor, lens: torch.Tensor, k: int, prefill_chunk: int):
        """generate()'s prompt forward: one shot, or in chunks of ``prefill_chunk`` positions."""
        if prefill_chunk > 0:
            return self.prefill_chunked(ids, lens, prefill_chunk, k)
        B, S = ids.shape
        pos = torch.arange(S, device=self.device, dtype=torch.int32).unsqueeze(0).expand(B, S).contiguous()
        return self.step(ids, pos, lens, decode=False, k=k)

    def gather_candidates(self, vals: torch.Tensor, idx: torch.Tensor):
        """X4 all-gather of every rank's local top-k -> ``[B, tp*k]`` values / ids (host tensors)."""
        allv = self.comm.all_gather(vals)
        alli = self.comm.all_gather(idx)
        B = vals.shape[0]
        return (allv.permute(1, 0, 2).reshape(B, -1).float().cpu(), alli.permute(1, 0, 2).reshape(B, -1).cpu())

    @staticmethod
    def pick_token(cv: torch.Tensor, ci: torch.Tensor, gp: GenParams, step: int) -> int:
        """One row's next token from its merged candidates -- the rule of the device pick kernel
        (ops.decode_pick): greedy = the first maximum; sampled = the ``top_k`` largest (ties in
        candidate order), softmax at ``temperature`` in fp32, the first cumulative weight above
        ``sample_uniform(seed, step)`` of the total."""
        if gp.top_k <= 1:
            return int(ci[int(cv.argmax())])
        k = min(gp.top_k, cv.shape[0], 64)
        v = cv.float()
        order = torch.sort(v, descending=True, stable=True).indices[:k]
        tv = v[order]
        w = torch.exp((tv - tv[0]) / max(gp.temperature, 1e-5))
        cdf = torch.cumsum(w, 0)
        thr = torch.tensor(sample_uniform(gp.seed, step), dtype=torch.float32) * cdf[-1]
        hit = (cdf > thr).nonzero()
        pick = int(hit[0, 0]) if hit.numel() else k - 1
        return int(ci[int(order[pick])])

    def ctx_bucket(self, max_ctx: Optional[int]) -> int:
        """Power-of-two context bound (>= 256, <= max_seq) a decode graph is captured for."""
        if max_ctx is None:
            return self.max_seq
        return min(self.max_seq, max(256, 1 << (max(1, int(max_ctx)) - 1).bit_length()))

    def _graph_ok(self, B: int) -> bool:
        """May the decode step for batch B be captured?  Always at tp == 1 / under a graph-safe
        comm; with the IPC all-reduce only while its B x hidden bf16 messages fit the one-shot
        buffer (larger ones would fall back to an uncapturable collective) unless RCCL capture
        is enabled."""
        if self.tp == 1 or getattr(self.comm, "graph_safe", False) or self._rccl_graphs:
            return True
        car = getattr(self.comm, "car", None)
        if car is None:
            return False
        probe = torch.empty(B * self.cfg.hidden, dtype=torch.bfloat16, device=car.device)
        return car.eligible(probe)  # one-shot or two-shot: both are in-stream kernels

    def _capture(self, ctx: int, warm, body):
        """Capture ``body()`` into a graph under the decode context bound ``ctx``, after two runs of
        ``warm()`` on a side stream (kernel selection, workspaces): ``(graph, body's result)``."""
        dev = self.device
        self._dec_ctx = ctx
        try:
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):
                    warm()
            torch.cuda.current_stream(dev).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            # thread_local: the RCCL watchdog thread polls its events while this thread captures
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                out = body()
        finally:
            self._dec_ctx = None
        return g, out

    def _warm_decode(self, B: int, k: int, ctx: int):
        """Warm-up of the device-resident steps' captures: a decode step + X4 gather on scratch inputs
        at position ctx - 1 (see :meth:`_decode_graph`); the shared per-B state is left alone."""
        dev = self.device
        tok = torch.zeros(B, 1, dtype=torch.int32, device=dev)
        pos = torch.full((B, 1), ctx - 1, dtype=torch.int32, device=dev)
        lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)

        def warm():
            self._gather_dev(*self.step(tok, pos, lens, decode=True, k=k))

        return warm

    def _decode_graph(self, B: int, k: int, ctx: int):
        """Captured decode step for batch B and context bound ctx (static token / position / length
        buffers).  The warm-up steps run at position ctx - 1: for a sequence being decoded under
        this bound that row is either the one the step about to replay writes anyway, or a future
        row that will be overwritten before anything reads it -- so graphs can be captured while
        sequences are in flight."""
        key = (B, k, ctx)
        if key in self._graphs:
            return self._graphs[key]
        dev = self.device
        tok = torch.zeros(B, 1, dtype=torch.int32, device=dev)
        pos = torch.full((B, 1), ctx - 1, dtype=torch.int32, device=dev)
        lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)

        def run():
            return self.step(tok, pos, lens, decode=True, k=k)

        g, (vals, idx) = self._capture(ctx, run, run)
        self._graphs[key] = (g, tok, pos, lens, vals, idx)
        return self._graphs[key]

    def decode_step(self, tok: torch.Tensor, cur: torch.Tensor, k: int, max_ctx: Optional[int] = None):
        """One decode step: token at position ``cur`` (attending to cur + 1 keys).  ``max_ctx``: a
        host-side bound on cur + 1 (e.g. prompt length + step), used to pick a tight split grid."""
        B = tok.shape[0]
        ctx = self.ctx_bucket(max_ctx)
        if self.use_graphs and self._graph_ok(B):
            g, t_s, p_s, l_s, v_s, i_s = self._decode_graph(B, k, ctx)
            if self.pages is not None:
                self.pages.device_table()  # the graph reads the table buffer in place
            t_s.copy_(tok.view(B, 1))
            p_s.copy_(cur.view(B, 1))
            l_s.copy_(cur.view(B) + 1)
            with tracing.range("llama.decode"):
                g.replay()
            return v_s, i_s
        self._dec_ctx = ctx
        try:
            return self.step(tok.view(B, 1).to(torch.int32), cur.view(B, 1), cur.view(B) + 1, decode=True, k=k)
        finally:
            self._dec_ctx = None

    @torch.no_grad()
    def generate(self, ids: torch.Tensor, lens: torch.Tensor, gp: GenParams, prefill_chunk: int = 0,
                 speculate: int = 0, drafter=None, spec_device: bool = False, spec_ngram=(3, 1)) -> torch.Tensor:
        """ids int ``[B, S]`` (right-padded), lens ``[B]`` -> generated ``[B, max_new_tokens]``.
        ``prefill_chunk = N > 0``: the prompts are prefilled N positions at a time
        (:meth:`prefill_chunked`) instead of in one forward.
        ``speculate = K > 0``: speculative decoding (models/speculative.py) -- each sequence proposes up to
        K draft tokens (``drafter(tokens, n_draft)``, default prompt lookup), one :meth:`verify_step`
        scores them and the sequence keeps the drafts that equal what it would have sampled anyway; a
        host loop, ``self.spec_stats`` counts its steps / drafted / accepted tokens.
        ``spec_device`` (with ``speculate``): the loop's verify step is one graph replay that also drafts
        (prompt lookup, n-grams ``spec_ngram = (max, min)``) and accepts on device
        (:meth:`serve_spec_graph`); the host reads one small block per step.  ``ValueError`` where the
        device loop is unavailable or with a ``drafter`` hook -- nothing falls back to the host loop."""
        B, S = ids.shape
        prefill_chunk = int(prefill_chunk)
        if prefill_chunk < 0:
            raise ValueError(f"prefill_chunk must be >= 0, got {prefill_chunk}")
        if prefill_chunk:
            self.check_prefill_chunk()
        speculate = int(speculate)
        if speculate < 0:
            raise ValueError(f"speculate must be >= 0, got {speculate}")
        if speculate:
            self.check_speculate(speculate)
        if spec_device:
            self.check_spec_device(speculate, drafter, k=max(1, min(gp.top_k, self.top_k_max)), Bv=B)
        if B > self.max_batch or S + gp.max_new_tokens > self.max_seq:
            raise ValueError("batch / sequence exceed the KV cache")
        if self.lora_loaded or gp.adapter != -1:
            self.set_batch_adapters(B, gp.adapter)
        lens_host = lens.detach().to("cpu")
        if lens_host.numel() != B or int(lens_host.min()) < 1 or int(lens_host.max()) > S:
            raise ValueError(f"lens must be in [1, {S}] for each of the {B} sequences")
        dev = self.device
        ids = ids.to(dev)
        lens = lens.to(dev).to(torch.int32)
        k = max(1, min(gp.top_k, self.top_k_max))
        if not speculate and self._device_loop_ok(B, k):
            return self._generate_device(ids, lens, gp, k, prefill_chunk)
        assigned = 0
        try:
            if self.pages is not None:  # batch row b = slot b, pages for the prompt + the generation budget
                for b in range(B):
                    self.pages.assign(b, S + gp.max_new_tokens)
                    assigned = b + 1
            vals, idx = self._prefill(ids, lens, k, prefill_chunk)
            if spec_device:
                return self._generate_speculative_device(ids, lens, lens_host, vals, idx, gp, k, speculate,
                                                         spec_ngram)
            if speculate:
                return self._generate_speculative(ids, lens_host, vals, idx, gp, k, speculate, drafter)
            out = []
            tok = self._sample_rows(vals, idx, gp, 0)
            out.append(tok)
            cur = lens.clone()
            for t in range(1, gp.max_new_tokens):
                # the new token sits at position cur; attention covers cur + 1 keys
                vals, idx = self.decode_step(tok.to(dev), cur, k, max_ctx=S + t)
                tok = self._sample_rows(vals, idx, gp, t)
                out.append(tok)
                cur = cur + 1
            return torch.stack(out, dim=1)
        finally:
            if self.pages is not None:  # also on OutOfPages part-way: release exactly the rows assigned
                for b in range(assigned):
                    self.pages.release(b)

    def _generate_speculative(self, ids: torch.Tensor, lens_host: torch.Tensor, vals, idx, gp: GenParams, k: int,
                              K: int, drafter) -> torch.Tensor:
        """generate()'s decode loop with K drafts per sequence and step: rows advance at their own rate
        and drop out of the verify batch (``slot_ids``) once they hold ``max_new_tokens``.  Every rank
        drafts from the same tokens and accepts from the same gathered candidates: no new message."""
        from . import speculative as SP

        B, S = ids.shape
        drafter = drafter or SP.prompt_lookup_draft
        ids_h = ids.to("cpu")
        seqs = [ids_h[b, : int(lens_host[b])].tolist() for b in range(B)]  # prompt + generated, per row
        first = self._sample_rows(vals, idx, gp, 0).tolist()
        outs: List[List[int]] = [[int(first[b])] for b in range(B)]
        cur = [int(x) for x in lens_host.tolist()]  # position of each row's last emitted token
        st = self.spec_stats = {"steps": 0, "drafted": 0, "accepted": 0}
        T = K + 1
        while True:
            rows = [b for b in range(B) if len(outs[b]) < gp.max_new_tokens]
            if not rows:
                break
            feeds = [SP.spec_feed(seqs[b] + outs[b], K, gp.max_new_tokens - len(outs[b]), drafter) for b in rows]
            ft = torch.zeros(len(rows), T, dtype=torch.int32)
            for j, f in enumerate(feeds):
                ft[j, : len(f)] = torch.tensor(f, dtype=torch.int32)
            n = torch.tensor([len(f) for f in feeds], dtype=torch.int32)
            past = torch.tensor([cur[b] for b in rows], dtype=torch.int32)
            v, i = self.verify_step(ft, past, n, k, slot_ids=torch.tensor(rows, dtype=torch.int32),
                                    max_ctx=int((past + n).max()))
            cv, ci = self.gather_candidates(v.reshape(len(rows) * T, -1), i.reshape(len(rows) * T, -1))
            st["steps"] += 1
            for j, b in enumerate(rows):
                e = len(outs[b])
                got = SP.accept(feeds[j], lambda t: self.pick_token(cv[j * T + t], ci[j * T + t], gp, e + t))
                outs[b] += got
                cur[b] += len(got)
                st["drafted"] += len(feeds[j]) - 1
                st["accepted"] += len(got) - 1
        return torch.tensor(outs, dtype=torch.int32)

    def _generate_speculative_device(self, ids: torch.Tensor, lens: torch.Tensor, lens_host: torch.Tensor, vals, idx,
                                     gp: GenParams, k: int, K: int, ngram) -> torch.Tensor:
        """:meth:`_generate_speculative` with the drafter and the acceptance inside the captured verify
        step (:meth:`serve_spec_graph`): batch row b is serving slot b, the verify batch is the rows that
        still owe tokens (as the host loop's), and one read-back of the per-slot ``(n, got, tokens)``
        blocks per step tells the host who is done and feeds ``spec_stats``."""
        B, S = ids.shape
        dev = self.device
        T = K + 1
        st = self.serve_state(self.max_batch, spec_T=T)
        sl = slice(0, B)
        st["prompt"][sl, :S] = ids.to(torch.int32)
        st["plen"][sl] = lens
        st["max_new"][sl] = int(gp.max_new_tokens)
        st["step"][sl] = 0
        st["topk"][sl] = int(gp.top_k)
        st["temp"][sl] = float(gp.temperature)
        st["seed"][sl] = int(gp.seed)
        st["pos"][sl] = lens - 1  # the pick advances them to (lens, lens + 1): the first decode position
        st["lens"][sl] = lens
        cv, ci = self._gather_dev(vals, idx)
        self.ops.decode_pick(cv, ci, st["tok"], st["pos"], st["lens"], st["step"], topk=st["topk"], temp=st["temp"],
                             seed=st["seed"], hist=st["hist"], rows=torch.arange(B, dtype=torch.int32, device=dev))
        stats = self.spec_stats = {"steps": 0, "drafted": 0, "accepted": 0}
        cur = [int(x) for x in lens_host.tolist()]  # position of each row's last emitted token
        have = [1] * B
        try:
            while True:
                rows = [b for b in range(B) if have[b] < gp.max_new_tokens]
                if not rows:
                    break
                max_ctx = max(cur[b] + 1 + max(0, min(K, gp.max_new_tokens - have[b] - 1)) for b in rows)
                g = self.serve_spec_graph(len(rows), T, k, self.ctx_bucket(max_ctx), ngram=ngram, eos=())
                st["spec_rows"][: len(rows)].copy_(torch.tensor(rows, dtype=torch.int32), non_blocking=True)
                if self.pages is not None:
                    self.pages.device_table()  # the graph reads the table buffer in place
                with tracing.range("llama.verify"):
                    g.replay()
                rb = st["spec_rb"].cpu().tolist()
                stats["steps"] += 1
                for b in rows:
                    n, got = rb[b][0], rb[b][1]
                    if got < 1:
                        raise RuntimeError(f"speculative step emitted nothing for row {b} (n = {n})")
                    have[b] += got
                    cur[b] += got
                    stats["drafted"] += n - 1
                    stats["accepted"] += got - 1
                if self.health_every > 0 and stats["steps"] % self.health_every == 0:
                    self.check_comm_health()
            self.check_comm_health()
            return st["hist"][sl, : gp.max_new_tokens].cpu()
        finally:  # the slots are idle again for a serving loop on this model
            st["pos"][sl] = 0
            st["lens"][sl] = 1

    # ---------------------------------------------------------------- device-resident decode loop
    def _gather_pad(self, k: int) -> int:
        return (-2 * k) % 4  # [B, 2k + pad] fp32 rows: a 16-B multiple per row (one-shot all-gather)

    def _device_loop_ok(self, B: int, k: int) -> bool:
        """May generate() run the X4 merge + token pick inside the captured decode step?"""
        if os.environ.get("MLS_DEVICE_PICK", "1") == "0":
            return False
        if not (self.backend == "fused" and self.device.type == "cuda" and self.use_graphs and self._graph_ok(B)):
            return False
        if self.tp * k > 512 or k > 64:
            return False
        if self.tp == 1 or getattr(self.comm, "graph_safe", False):
            return True
        car = getattr(self.comm, "car", None)
        if car is not None:  # + the serving step's control row (serve_graph)
            return (B + 1) * (2 * k + self._gather_pad(k)) * 4 <= car.cap
        return self._rccl_graphs and not getattr(self.comm, "host_staged", False)

    def _spec_device_ok(self, Bv: int, T: int, k: int) -> bool:
        """May a verify step of ``Bv`` sequences x ``T`` positions draft, gather and accept inside its
        captured graph?  What :meth:`_device_loop_ok` asks, for the ``Bv * T + 1``-row gather."""
        if os.environ.get("MLS_DEVICE_PICK", "1") == "0":
            return False
        if not (self.backend == "fused" and self.device.type == "cuda" and self.use_graphs
                and self._graph_ok(Bv * T)):
            return False
        if self.tp * k > 512 or k > 64:
            return False
        if self.tp == 1 or getattr(self.comm, "graph_safe", False):
            return True
        car = getattr(self.comm, "car", None)
        if car is not None:
            return (Bv * T + 1) * (2 * k + self._gather_pad(k)) * 4 <= car.cap
        return self._rccl_graphs and not getattr(self.comm, "host_staged", False)

    def check_spec_device(self, speculate: int, drafter=None, k: Optional[int] = None, Bv: Optional[int] = None) -> None:
        """``spec_device`` (the verify step drafts and accepts on device): raises ``ValueError`` without
        ``speculate``, with a host ``drafter`` hook, for what :meth:`check_speculate` refuses and wherever
        the device loop is unavailable -- nothing falls back to the host loop."""
        speculate = int(speculate)
        if speculate < 1:
            raise ValueError("spec_device needs speculate >= 1")
        if drafter is not None:
            raise ValueError("spec_device drafts by prompt lookup inside the captured step: a drafter callable "
                             "(a host hook) cannot run there")
        self.check_speculate(speculate)
        T = speculate + 1
        Bv = max(1, 16 // T) if Bv is None else int(Bv)
        k = self.top_k_max if k is None else int(k)
        if not self._spec_device_ok(Bv, T, k):
            raise ValueError("spec_device needs the device-resident loop: the fused backend on a GPU with graphs on, "
                             f"MLS_DEVICE_PICK != 0, tp * k <= 512 and a {Bv * T + 1}-row candidate gather that "
                             f"fits the one-shot buffer (backend {self.backend}, device {self.device.type}, "
                             f"graphs {bool(self.use_graphs)}, tp {self.tp}, k {k})")

    def _gather_dev(self, vals: torch.Tensor, idx: torch.Tensor, ctl: Optional[torch.Tensor] = None):
        """X4 on device: every rank's [B, k] candidates -> ([tp, B, k] f32, [tp, B, k] i32), one
        collective (values and ids packed in one fp32 row); graph-capturable.  ``ctl`` (int32
        [CTL_WORDS], optional): one more row rides the same collective, and the call returns a third
        value, RANK 0's ctl words (int32 [CTL_WORDS]) -- the serving loop's next-iteration header
        (models/llama_serving.py), with no collective of its own."""
        if self.tp == 1:
            if ctl is not None:
                return vals.unsqueeze(0), idx.unsqueeze(0), ctl.clone()
            return vals.unsqueeze(0), idx.unsqueeze(0)
        B, k = vals.shape
        pad = self._gather_pad(k)
        parts = [vals.float(), idx.view(torch.float32)]
        if pad:
            parts.append(torch.zeros(B, pad, device=vals.device, dtype=torch.float32))
        pack = torch.cat(parts, dim=1)
        if ctl is not None:  # W = 2k + pad >= 4 >= CTL_WORDS fp32 columns
            W = pack.shape[1]
            row = torch.zeros(1, W, device=vals.device, dtype=torch.float32)
            row[0, : ctl.numel()] = ctl.view(torch.float32)
            pack = torch.cat([pack, row], dim=0)
        pack = pack.contiguous()
        car = getattr(self.comm, "car", None)
        if car is not None and car.gather_eligible(pack):
            with tracing.range("tp.all_gather"):
                g = car.all_gather(pack)
        elif getattr(self.comm, "graph_safe", False):
            g = self.comm.all_gather(pack)
        else:
            g = torch.empty((self.tp, *pack.shape), device=pack.device, dtype=pack.dtype)
            with tracing.range("tp.all_gather"):
                dist.all_gather_into_tensor(g, pack, group=self.comm.group)
        if ctl is not None:
            c0 = g[0, B, : ctl.numel()].contiguous().view(torch.int32)
            g = g[:, :B]
            return g[..., :k].contiguous(), g[..., k: 2 * k].contiguous().view(torch.int32), c0
        return g[..., :k].contiguous(), g[..., k: 2 * k].contiguous().view(torch.int32)

    def _dev_buffers(self, B: int):
        st = self._dev_state.get(B)
        if st is None:
            dev = self.device
            z = lambda dt: torch.zeros(B, device=dev, dtype=dt)  # noqa: E731
            st = (z(torch.int32), z(torch.int32), z(torch.int32), z(torch.int32),  # tok, pos, lens, step
                  z(torch.int32), torch.ones(B, device=dev, dtype=torch.float32), z(torch.int64),  # topk, temp, seed
                  torch.zeros(B, self.max_seq, device=dev, dtype=torch.int32))  # hist
            self._dev_state[B] = st
        return st

    def _decode_graph_dev(self, B: int, k: int, ctx: int) -> torch.cuda.CUDAGraph:
        """Captured decode step + X4 gather + on-device pick for batch B / context bound ctx: reads
        tok / pos / lens of the shared per-B state and advances them for the next replay."""
        key = (B, k, ctx)
        g = self._dev_graphs.get(key)
        if g is not None:
            return g
        tok, pos, lens, step, topk, temp, seed, hist = self._dev_buffers(B)

        def body():
            v, i = self.step(tok.view(B, 1), pos.view(B, 1), lens, decode=True, k=k)
            cv, ci = self._gather_dev(v, i)
            self.ops.decode_pick(cv, ci, tok, pos, lens, step, topk=topk, temp=temp, seed=seed, hist=hist)

        g, _ = self._capture(ctx, self._warm_decode(B, k, ctx), body)
        self._dev_graphs[key] = g
        return g

    # ---------------------------------------------------------------- serving (ContinuousLlama) on device
    def serve_state(self, B: int, spec_T: int = 0) -> Dict[str, torch.Tensor]:
        """Per-slot device state of the continuous-batching decode loop (models/llama_serving.py):
        ``E`` int32 [2, B] is the one per-iteration read-back -- row 0 the prefill picks of the
        iteration's new sequences, row 1 (= ``tok``, the decode graph's input and output token) the
        decode picks; ``active`` masks idle slots out of the pick (they decode a dummy token into
        their own cache row / the scratch page and keep pos 0).  ``E_all`` = ``E`` followed by
        ``ctl_out`` (int32 [CTL_WORDS]): rank 0's ``ctl_in`` as the decode step's gather carried it
        (the next iteration's header at TP > 1), and ``err_out`` (int32 [1]): this rank's one-shot
        collectives' sticky peer-timeout word after the step -- all read back in the same copy.
        ``spec_T = K + 1`` (speculation on device, :meth:`serve_spec_graph`): the state also holds each slot's
        tokens for the drafter -- ``prompt`` int32 [B, max_seq] / ``plen``, ``hist`` int32 [B, max_seq] (the
        emitted tokens, ``step`` of them) and ``max_new`` -- the verify rows' slots ``spec_rows``, and the
        read-back block ``spec_rb`` int32 [B, spec_T + 2] = (n fed, got, the got tokens) per slot, appended to
        ``E_all`` behind ``err_out``: still one copy per iteration.  A state built without (or for a smaller
        ``spec_T``) is rebuilt, with the graphs that baked its addresses; ``spec_T = 0`` returns what exists."""
        st = self._serve.get(B)
        if st is not None and int(spec_T) > st.get("spec_T", 0):
            for key in [q for q in self._dev_graphs if isinstance(q[0], str) and q[0].startswith("serve")]:
                del self._dev_graphs[key]
            st = None
        if st is None:
            dev = self.device
            T = int(spec_T)
            z = lambda dt: torch.zeros(B, device=dev, dtype=dt)  # noqa: E731
            base = 2 * B + CTL_WORDS + 1
            E_all = torch.zeros(base + (B * (T + 2) if T else 0), device=dev, dtype=torch.int32)
            E = E_all[: 2 * B].view(2, B)
            st = {"E": E, "E_all": E_all, "ctl_out": E_all[2 * B: 2 * B + CTL_WORDS],
                  "err_out": E_all[2 * B + CTL_WORDS: base],
                  "ctl_in": torch.zeros(CTL_WORDS, device=dev, dtype=torch.int32),
                  "tok": E[1], "pos": z(torch.int32), "lens": torch.ones(B, device=dev, dtype=torch.int32),
                  "step": z(torch.int32), "topk": torch.ones(B, device=dev, dtype=torch.int32),
                  "temp": torch.ones(B, device=dev, dtype=torch.float32), "seed": z(torch.int64),
                  "active": z(torch.int32)}
            if T:
                st.update(spec_T=T, spec_rb=E_all[base:].view(B, T + 2), plen=z(torch.int32), max_new=z(torch.int32),
                          prompt=torch.zeros(B, self.max_seq, device=dev, dtype=torch.int32),
                          hist=torch.zeros(B, self.max_seq, device=dev, dtype=torch.int32),
                          spec_rows=torch.zeros(max(B, 16), device=dev, dtype=torch.int32))
            self._serve[B] = st
        return st

    def serve_graph(self, B: int, k: int, ctx: int, hist: bool = False) -> torch.cuda.CUDAGraph:
        """Captured serving decode step over all B slots: forward + X4 gather + the on-device pick
        of the ACTIVE slots (``ops.decode_pick(active=...)``), advancing their state in place.
        ``hist`` (speculation on device): the pick also appends each token to the slot's ``hist`` row, so
        a later verify step drafts from the complete history; captured and keyed separately."""
        key = ("serve_hist" if hist else "serve", B, k, ctx)
        g = self._dev_graphs.get(key)
        if g is not None:
            return g
        st = self.serve_state(B)

        def body():
            v, i = self.step(st["tok"].view(B, 1), st["pos"].view(B, 1), st["lens"], decode=True, k=k)
            cv, ci, c0 = self._gather_dev(v, i, ctl=st["ctl_in"])
            st["ctl_out"].copy_(c0)
            car = getattr(self.comm, "car", None)
            if car is not None:  # did a peer wait of this step (or an earlier one) time out?
                car.error_peek(st["err_out"])
            self.ops.decode_pick(cv, ci, st["tok"], st["pos"], st["lens"], st["step"], topk=st["topk"],
                                 temp=st["temp"], seed=st["seed"], active=st["active"],
                                 hist=st["hist"] if hist else None)

        g, _ = self._capture(ctx, self._warm_decode(B, k, ctx), body)
        self._dev_graphs[key] = g
        return g

    def serve_spec_graph(self, Bv: int, T: int, k: int, ctx: int, ngram=(3, 1), eos=None) -> torch.cuda.CUDAGraph:
        """Captured speculative step of the ``Bv`` slots listed in ``spec_rows[:Bv]`` of the serving state
        (:meth:`serve_state` with ``spec_T = T``): ``ops.spec_draft`` writes the verify forward's inputs
        from each slot's own tokens, the ``all_rows`` forward scores the ``Bv * T`` rows, the X4 gather
        carries the control row as :meth:`serve_graph`'s does, and ``ops.spec_accept`` picks each fed row,
        keeps the drafts that equal the picks and advances the slots in place -- one replay, then one
        ``E_all`` copy.  ``ngram = (max, min)`` of the prompt lookup; ``eos``: ids that end a sequence
        (default the model's).  Warm-up runs the forward on scratch inputs with ``lens == past`` (every
        row is padding: no cache row is written, no slot state touched)."""
        eos = tuple(sorted(self.cfg.eos_ids if eos is None else eos))
        key = ("serve_spec", Bv, T, k, ctx, self.verify_attn, tuple(ngram), eos)
        hit = self._dev_graphs.get(key)
        if hit is not None:
            return hit[0]
        B = self.max_batch
        st = self.serve_state(B, spec_T=T)
        if st["spec_T"] != T:
            raise ValueError(f"the serving state was built for {st['spec_T']} verify positions, not {T}")
        dev = self.device
        zi = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)  # noqa: E731
        ids, n, past, lens = zi(Bv, T), zi(Bv), zi(Bv), zi(Bv)
        rows = st["spec_rows"][:Bv]
        off = torch.arange(T, dtype=torch.int32, device=dev).unsqueeze(0)
        eos_t = torch.tensor(eos, dtype=torch.int32, device=dev) if eos else None
        w_ids, w_zero, w_rows = zi(Bv, T), zi(Bv), torch.arange(Bv, dtype=torch.int32, device=dev) % B
        if self.pages is not None:
            self.pages.device_table()

        def warm():
            v, i = self.step(w_ids, w_zero.unsqueeze(1) + off, w_zero, decode=False, k=k, slot_ids=w_rows, past=w_zero,
                             all_rows=True)
            self._gather_dev(v, i)

        def body():
            self.ops.spec_draft(rows, st["prompt"], st["plen"], st["hist"], st["step"], st["max_new"], st["pos"], ids,
                                n, past, lens, K=T - 1, max_ngram=int(ngram[0]), min_ngram=int(ngram[1]))
            v, i = self.step(ids, past.unsqueeze(1) + off, lens, decode=False, k=k, slot_ids=rows, past=past,
                             all_rows=True)
            cv, ci, c0 = self._gather_dev(v, i, ctl=st["ctl_in"])
            st["ctl_out"].copy_(c0)
            car = getattr(self.comm, "car", None)
            if car is not None:  # did a peer wait of this step (or an earlier one) time out?
                car.error_peek(st["err_out"])
            self.ops.spec_accept(cv, ci, ids, n, rows, st["tok"], st["pos"], st["lens"], st["step"], st["hist"],
                                 st["spec_rb"], topk=st["topk"], temp=st["temp"], seed=st["seed"], eos=eos_t)

        # this graph's own split-KV workspace: the first warm-up step sizes it, the capture bakes its address
        self._ver_ws_graph = torch.empty(0, device=dev, dtype=torch.float32)
        try:
            g, _ = self._capture(ctx, warm, body)
        finally:
            ws, self._ver_ws_graph = self._ver_ws_graph, None
        # the buffers stay referenced: the captured launches read / write them at every replay
        self._dev_graphs[key] = (g, ids, n, past, lens, off, eos_t, ws)
        return g

    def check_comm_health(self) -> None:
        """Collective (same decode step on every rank): did any one-shot collective lose a peer
        since the last check?  On an error every rank resets the device protocol, drops the IPC
        path (RCCL from now on) and its captured steps, and raises :class:`TPCommError`."""
        car = getattr(self.comm, "car", None)
        if self.tp == 1 or car is None:
            return
        err = car.errors()
        backend = dist.get_backend(self.comm.group)
        flag = torch.tensor([err], dtype=torch.int32, device=self.device if backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.comm.group)
        if int(flag.item()):
            car.reset()
            self.comm.car = None
            self._graphs.clear()
            self._ver_graphs.clear()
            self._dev_graphs.clear()
            raise TPCommError("a tensor-parallel peer missed a one-shot collective; falling back to RCCL")

    def _generate_device(self, ids: torch.Tensor, lens: torch.Tensor, gp: GenParams, k: int,
                         prefill_chunk: int = 0) -> torch.Tensor:
        """generate() with every decode step a graph replay that also merges the ranks' candidates
        and picks the next token on device (X4 + P4): no host round trip until the end (and the
        comm-health check every ``health_every`` steps)."""
        B, S = ids.shape
        dev = self.device
        tok, pos, lens_s, step, topk, temp, seed, hist = self._dev_buffers(B)
        step.zero_()
        topk.fill_(int(gp.top_k))
        temp.fill_(float(gp.temperature))
        seed.fill_(int(gp.seed))
        assigned = 0
        try:
            if self.pages is not None:
                for b in range(B):
                    self.pages.assign(b, S + gp.max_new_tokens)
                    assigned = b + 1
            vals, idx = self._prefill(ids, lens, k, prefill_chunk)
            cv, ci = self._gather_dev(vals, idx)
            pos.copy_(lens - 1)  # the pick advances them to (lens, lens + 1): the first decode position
            lens_s.copy_(lens)
            self.ops.decode_pick(cv, ci, tok, pos, lens_s, step, topk=topk, temp=temp, seed=seed, hist=hist)
            for t in range(1, gp.max_new_tokens):
                g = self._decode_graph_dev(B, k, self.ctx_bucket(S + t))
                if self.pages is not None:
                    self.pages.device_table()  # the graph reads the table buffer in place
                with tracing.range("llama.decode"):
                    g.replay()
                if self.health_every > 0 and t % self.health_every == 0:
                    self.check_comm_health()
            self.check_comm_health()
            return hist[:, : gp.max_new_tokens].cpu()
        finally:
            if self.pages is not None:
                for b in range(assigned):
                    self.pages.release(b)

    def _sample_rows(self, vals, idx, gp: GenParams, step: int) -> torch.Tensor:
        cv, ci = self.gather_candidates(vals, idx)
        return torch.tensor([self.pick_token(cv[b], ci[b], gp, step) for b in range(cv.shape[0])],
                            dtype=torch.int32)
