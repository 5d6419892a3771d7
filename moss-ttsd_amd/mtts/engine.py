"""Python handle on the HIP engine: device memory and streams come from
PyTorch-ROCm, everything that computes lives in libmtts.so."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import ban_spec, bias_spec, capi, warp_spec


def sampler_cfgs(layers=None, do_samples=None):
    """generation_config.layers / do_samples (reference modeling_asteroid.py:95-106) -> MttsSamplerCfg[8]."""
    arr = (capi.MttsSamplerCfg * 8)()
    for i in range(8):
        lc = (layers[i] if layers and i < len(layers) else {}) or {}
        s = arr[i]
        s.do_sample = 1 if (do_samples and do_samples[i]) else 0
        s.top_k = int(lc.get("top_k") or 0)
        tp = lc.get("top_p")
        s.top_p = float(tp) if tp is not None else 0.0
        s.one_minus_top_p = float(np.float32(1.0 - tp)) if tp is not None else 0.0
        t = lc.get("temperature")
        s.temperature = float(t) if t is not None else 0.0
        rp = lc.get("repetition_penalty")
        s.repetition_penalty = float(rp) if rp is not None else 0.0
    return arr


def sampler_floors(layers=None, do_samples=None):
    """The probability floors of the same per-channel dicts -> MttsSamplerFloors[8], or None when no sampled channel sets
    one (the run then launches what it launched before floors existed).  Keys `min_p`, `epsilon_cutoff`, `eta_cutoff`
    (HF's MinP / Epsilon / EtaLogitsWarper; mtts/warp_spec.py states the rule): this engine's extension of the reference's
    four per-channel keys.  None or 0 = absent; a greedy channel's are ignored, like its top_k / top_p.  ValueError, naming
    the channel, for a value outside HF's range."""
    arr, on = (capi.MttsSamplerFloors * 8)(), False
    for i in range(8):
        lc = (layers[i] if layers and i < len(layers) else {}) or {}
        f = warp_spec.floors_of(lc, f"layers[{i}]: ")
        if do_samples and do_samples[i]:
            arr[i].min_p, arr[i].epsilon_cutoff, arr[i].eta_cutoff, arr[i].sqrt_eta_cutoff = f
            on = on or any(v > 0.0 for v in f[:3])
    return arr if on else None


def sampler_typical(layers=None, do_samples=None):
    """typical_p of the same per-channel dicts -> float[8], or None when no sampled channel sets one (the run then launches
    what it launched before).  Key `typical_p` (HF's TypicalLogitsWarper; mtts/warp_spec.py states the rule).  None or 1.0 =
    absent; a greedy channel's is ignored.  ValueError, naming the channel, for anything not strictly inside (0, 1)."""
    arr, on = (C.c_float * 8)(), False
    for i in range(8):
        lc = (layers[i] if layers and i < len(layers) else {}) or {}
        t = warp_spec.typical_of(lc, f"layers[{i}]: ")
        if do_samples and do_samples[i]:
            arr[i] = t
            on = on or t > 0.0
    return arr if on else None


def sampler_bans(layers=None):
    """The hard bans of the same per-channel dicts -> MttsSamplerBans[8], or None when no channel sets one (the run then
    launches and allocates what it did before bans existed).  Keys `no_repeat_ngram_size` (1..16), `suppress_tokens` (a
    list of ids >= 0; those outside the channel's vocabulary are ignored) and `min_new_tokens` (HF's NoRepeatNGram /
    SuppressTokens / MinNewTokensLength processors; mtts/ban_spec.py states the rule).  None, 0 or [] = absent.  They are
    processors, not warpers: a greedy channel applies them like a sampled one.  ValueError, naming the channel, for a bad
    value.  The array keeps the id lists alive (`_keep`)."""
    arr, on, keep = (capi.MttsSamplerBans * 8)(), False, []
    for i in range(8):
        lc = (layers[i] if layers and i < len(layers) else {}) or {}
        n, m, sup = ban_spec.bans_of(lc, f"layers[{i}]: ")
        ids = (C.c_int32 * max(len(sup), 1))(*sup)
        keep.append(ids)
        arr[i].no_repeat_ngram_size, arr[i].min_new_tokens, arr[i].n_suppress = n, m, len(sup)
        arr[i].suppress = C.cast(ids, C.POINTER(C.c_int32))
        on = on or n > 0 or m > 0 or len(sup) > 0
    arr._keep = keep
    return arr if on else None


def sampler_bias(layers=None, eos_token_id=None):
    """The sequence rules and step-conditioned bans of the same per-channel dicts -> MttsSamplerBias[8], or None when no
    channel sets one (the run then launches and allocates what it did before they existed).  Keys `sequence_bias` (HF's dict
    or list form), `bad_words_ids` (lists equal to [eos_token_id] are dropped, as HF drops them), `min_length` and
    `begin_suppress_tokens` (HF's SequenceBias / NoBadWords / MinLength / SuppressTokensAtBegin processors; mtts/bias_spec.py
    states the rule).  None, 0, {} or [] = absent.  Processors, not warpers: a greedy channel applies them like a sampled
    one.  ValueError, naming the channel, for a bad value.  The array keeps its lists alive (`_keep`)."""
    arr, on, keep = (capi.MttsSamplerBias * 8)(), False, []
    for i in range(8):
        lc = (layers[i] if layers and i < len(layers) else {}) or {}
        rules, m, begin = bias_spec.bias_of(lc, f"layers[{i}]: ", eos_token_id)
        flat = [t for ids, _ in rules for t in ids]
        lens = (C.c_int32 * max(len(rules), 1))(*[len(ids) for ids, _ in rules])
        ids = (C.c_int32 * max(len(flat), 1))(*flat)
        beta = (C.c_float * max(len(rules), 1))(*[b for _, b in rules])
        beg = (C.c_int32 * max(len(begin), 1))(*begin)
        keep.append((lens, ids, beta, beg))
        arr[i].n_rules, arr[i].min_length, arr[i].n_begin_suppress = len(rules), m, len(begin)
        arr[i].rule_len = C.cast(lens, C.POINTER(C.c_int32))
        arr[i].rule_ids = C.cast(ids, C.POINTER(C.c_int32))
        arr[i].rule_bias = C.cast(beta, C.POINTER(C.c_float))
        arr[i].begin_suppress = C.cast(beg, C.POINTER(C.c_int32))
        on = on or bool(rules) or m > 0 or bool(begin)
    arr._keep = keep
    return arr if on else None


def rope_tables(head_dim, theta, rows, device, dtype=torch.bfloat16):
    """cos/sin exactly as Qwen3RotaryEmbedding.forward builds them (transformers
    modeling_qwen3.py:96-138): fp32 inv_freq, fp32 outer product, cos/sin, cast to the model dtype."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float) / head_dim))
    pos = torch.arange(rows, dtype=torch.float)
    freqs = (inv_freq[:, None] @ pos[None, :]).transpose(0, 1)            # [rows, 64]
    return (freqs.cos().to(dtype).contiguous().to(device),
            freqs.sin().to(dtype).contiguous().to(device))


class Engine:
    def __init__(self, cfg: dict, max_batch: int, max_seq_len: int, device="cuda:0", kv_pool_pages: int = 0, dtype="bf16"):
        """dtype "bf16" (the reference default) or "fp32" (`inference.py --dtype fp32`: fp32 weights, arithmetic,
        K/V pages and logits -- the strict-parity mode, plain HBM-bound kernels)."""
        if dtype not in ("bf16", "fp32", "fp16"):
            raise NotImplementedError(f"dtype {dtype!r} is not built (bf16, fp32, fp16)")
        self.dtype = dtype
        # "fp16" (`inference.py --dtype fp16`): the fp32 engine with fp16 rounding points; its tensors are fp32 holding fp16 values
        self.tdtype = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.model_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(dtype, torch.float32)
        if not torch.cuda.is_available():
            raise capi.MttsError("no GPU visible: the mtts engine only runs on MI355X (no CPU fallback)")
        self.cfg = cfg
        self.device = torch.device(device)
        self.lib = capi.lib()
        c = capi.MttsConfig()
        for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                  "num_key_value_heads", "head_dim", "channels", "speech_vocab_size", "speech_pad_token",
                  "eos_token_id"):
            setattr(c, k, int(cfg[k]))
        c.speech_range_lo, c.speech_range_hi = int(cfg["speech_token_range"][0]), int(cfg["speech_token_range"][1])
        c.max_position = int(max_seq_len) + 24
        c.rms_norm_eps = float(cfg["rms_norm_eps"])
        c.max_batch, c.max_seq_len = int(max_batch), int(max_seq_len)
        c.kv_pool_pages = int(kv_pool_pages)          # 0: every slot can reach max_seq_len at once
        c.dtype = {"bf16": 0, "fp32": 1, "fp16": 2}[dtype]
        self._h = C.c_void_p()
        self._topk = 0
        capi.check(self.lib.mtts_engine_create(C.byref(c), self.device.index or 0, C.byref(self._h)))
        cos, sin = (t.to(self.tdtype) for t in rope_tables(cfg["head_dim"], float(cfg["rope_theta"]), c.max_position,
                                                           self.device, self.model_dtype))
        torch.cuda.synchronize(self.device)
        capi.check(self.lib.mtts_bind_rope(self._h, cos.data_ptr(), sin.data_ptr(), c.max_position, None))
        torch.cuda.synchronize(self.device)

    def close(self):
        """-> mtts_engine_destroy's code: MTTS_OK, or MTTS_EHIP when freeing one of the engine's buffers failed."""
        rc = 0
        if self._h:
            rc = self.lib.mtts_engine_destroy(self._h)
            self._h = C.c_void_p()
        return rc

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights -----------------------------------------------------------
    def bind(self, name: str, tensor: torch.Tensor):
        t = tensor.to(device=self.device).to(self.model_dtype).to(self.tdtype).contiguous()      # (cast like model.to(dtype) casts)
        rows, cols = (t.shape[0], t.shape[1]) if t.dim() == 2 else (t.shape[0], 1)
        capi.check(self.lib.mtts_bind_weight(self._h, name.encode(), t.data_ptr(), rows, cols, None))
        torch.cuda.synchronize(self.device)     # the engine has packed its own copy; `t` may go

    def bind_lora(self, name: str, base, A, B, scaling, sync=True):
        """bind(name, merged) with the LoRA merge done on the device on the way into the engine's layout (include/mtts.h:
        mtts_bind_weight_lora): merged = round(base + ((B @ A), r terms in ascending order, fp32) * scaling).  base as
        bind() takes it; A = lora_A.weight [r, in], B = lora_B.weight [out, r] (widened to fp32); scaling one fp32 value.
        sync=False: the call is only enqueued (on the device's default stream, like the copies torch made for it); a caller
        that binds many matrices synchronises once after the last."""
        as_t = lambda v: torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
        t = as_t(base).to(device=self.device).to(self.model_dtype).to(self.tdtype).contiguous()
        a, b = (as_t(v).to(device=self.device, dtype=torch.float32).contiguous() for v in (A, B))
        if t.dim() != 2 or a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1] or tuple(t.shape) != (b.shape[0], a.shape[1]):
            raise ValueError(f"{name}: base {tuple(t.shape)}, lora_A {tuple(a.shape)}, lora_B {tuple(b.shape)} are not [out, in], [r, in], [out, r]")
        capi.check(self.lib.mtts_bind_weight_lora(self._h, name.encode(), t.data_ptr(), t.shape[0], t.shape[1], a.data_ptr(),
                                                  b.data_ptr(), int(a.shape[0]), C.c_float(float(scaling)), None))
        if sync:
            torch.cuda.synchronize(self.device)     # the engine holds the merged matrix; the three tensors may go

    def load_bank_adapter(self, idx, tensors, scaling):
        """Adapter `idx` (0..15) of the engine's bank of resident, UNMERGED adapters (include/mtts.h: mtts_adapter_load):
        tensors {engine weight name: (A [r, in], B [out, r])} as adapters.read_peft_dir returns them, r <= 64; scaling one
        fp32 value.  Replaces whatever `idx` held.  A row that names it (row_adapters= / adapter=) computes
        W x + scaling * B (A x) in every projection the adapter targets; the bound weights stay as they are.  bf16 only."""
        self.clear_bank_adapter(idx)
        as_t = lambda v: torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
        for name, (A, B) in tensors.items():
            a, b = (as_t(v).to(device=self.device, dtype=torch.float32).contiguous() for v in (A, B))
            if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1]:
                raise ValueError(f"{name}: lora_A {tuple(a.shape)} and lora_B {tuple(b.shape)} are not [r, in] and [out, r]")
            torch.cuda.synchronize(self.device)         # torch's copies have landed; the call copies and drains its stream
            capi.check(self.lib.mtts_adapter_load(self._h, int(idx), name.encode(), a.data_ptr(), b.data_ptr(), b.shape[0], a.shape[1],
                                                  int(a.shape[0]), C.c_float(float(scaling)), None))

    def clear_bank_adapter(self, idx):
        capi.check(self.lib.mtts_adapter_clear(self._h, int(idx)))

    def _set_row_adapters(self, row_adapters, B):
        if row_adapters is not None:
            r = np.ascontiguousarray([-1 if a is None else int(a) for a in row_adapters], dtype=np.int32)
            if r.shape != (B,):
                raise ValueError(f"row_adapters has {r.size} entries, the batch has {B} prompts")
            capi.check(self.lib.mtts_set_row_adapters(self._h, r.ctypes.data, B))

    def bind_state_dict(self, sd):
        for k, v in sd.items():
            if k.startswith("lm_heads.") or k.endswith("embed_tokens.weight"):
                continue
            if isinstance(v, np.ndarray):
                v = torch.from_numpy(v)
            self.bind(k, v)
        capi.check(self.lib.mtts_weights_ready(self._h))

    # ---- generation --------------------------------------------------------
    @staticmethod
    def _host_inputs(input_ids, attention_mask):
        ids = np.ascontiguousarray(np.asarray(input_ids.cpu() if torch.is_tensor(input_ids) else input_ids), dtype=np.int64)
        m = attention_mask.cpu().numpy() if torch.is_tensor(attention_mask) else np.asarray(attention_mask)
        m = np.ascontiguousarray((m > 0).astype(np.uint8))
        assert ids.ndim == 3 and ids.shape[2] == 8 and m.shape == ids.shape[:2]
        return ids, m

    def _set_row_ids(self, row_ids, B):
        if row_ids is not None:
            r = np.ascontiguousarray(row_ids, dtype=np.int32)
            assert r.shape == (B,)
            capi.check(self.lib.mtts_set_row_ids(self._h, r.ctypes.data, B))

    def _set_takes(self, takes):
        takes = int(takes)
        if takes < 1:
            raise ValueError(f"takes must be >= 1 (got {takes})")
        capi.check(self.lib.mtts_set_takes(self._h, takes))
        return takes

    def _set_floors_and_bans(self, layers, do_samples):
        """One-shots like takes: the floors and the hard bans of `layers` for the run that starts next, or none
        (mtts_set_sampler_floors, mtts_set_sampler_typical, mtts_set_sampler_bans, mtts_set_sampler_bias).  All are
        marshalled first: a bad value leaves nothing pending."""
        floors, typical, bans = sampler_floors(layers, do_samples), sampler_typical(layers, do_samples), sampler_bans(layers)
        bias = sampler_bias(layers, self.cfg.get("eos_token_id"))
        capi.check(self.lib.mtts_set_sampler_floors(self._h, floors))
        capi.check(self.lib.mtts_set_sampler_typical(self._h, typical))
        capi.check(self.lib.mtts_set_sampler_bans(self._h, bans))
        capi.check(self.lib.mtts_set_sampler_bias(self._h, bias))

    def set_output_scores(self, on):
        """Sticky engine switch, read when the next run begins (begin / generate / sched_open): per-token
        log-probabilities (include/mtts.h: mtts_set_output_scores).  MttsError(ESTATE) when it would change while rows of
        a run are still unfinished -- also a run that was abandoned mid-flight (begin + a few steps): end that one with
        sched_open(slots, gen_cap, output_scores=<its setting>) first.  begin / generate / sched_open call this with their
        own `output_scores` argument, so the same holds for them."""
        capi.check(self.lib.mtts_set_output_scores(self._h, 1 if on else 0))

    def set_top_logprobs(self, k):
        """Sticky engine switch like set_output_scores, and independent of it (include/mtts.h: mtts_set_top_logprobs): k = 0
        off, 1..16 the number of most probable tokens kept per decision.  begin / generate / sched_open call this with
        their own `top_logprobs` argument."""
        capi.check(self.lib.mtts_set_top_logprobs(self._h, int(k)))
        self._topk = int(k)             # (the run that starts next; the read functions size their buffers by it)

    def generate(self, input_ids, attention_mask, max_length, layers=None, do_samples=None, seed=0, forced=None,
                 forced_as_draw=False, row_ids=None, takes=1, output_scores=False, row_adapters=None, top_logprobs=0):
        """forced (verification hook): int64 [B,G,8] full sequences of a reference run.  -> (ids, decisions [steps,B,8]).
        forced_as_draw: the forced row replaces each step's raw draw before the state machine (replay of a SAMPLED
        run); decisions are then the raw draws.  forced_as_draw="all": also for rows that max_length has cut off (the
        reference keeps evaluating them; scripted tests of chained resurrections).
        takes: sampled takes per prompt (HF num_return_sequences): B*takes rows, row b*takes+j is take j of prompt b,
        equal to the run of the repeat-interleaved batch; row_ids then has B*takes entries.
        output_scores: the return value gains a last element lp, float32 [B*takes, G, 8] aligned with ids[:, T-7:]:
        log_softmax(processed scores)[the sampler's decision], NaN where the appended token is not a model decision
        (teacher forcing, EOS flush, finished-row padding).
        row_adapters: one bank index per PROMPT (load_bank_adapter), -1 or None = no adapter; a prompt's takes inherit it.
        top_logprobs=k (1..16): the return value gains, after lp, a tuple (logprobs float32 [B*takes, G, 8], top_ids int32
        [B*takes, G, 8, k], top_logprobs float32 [B*takes, G, 8, k]): the model's own distribution at every decision --
        log_softmax of the step's raw logits (hard-coded masks only; no penalty, temperature, top-k, top-p) at the
        sampler's decision and at the k most probable tokens (descending logit, ascending id among equals); NaN / -1
        exactly where lp is NaN."""
        ids, m = self._host_inputs(input_ids, attention_mask)
        B, T, _ = ids.shape
        R = B * int(takes)
        cap = int(max_length) + 6 * R + 8  # flushes that start at / run past max_length, chained (include/mtts.h: mtts_generate)
        self._B = R
        mode = 0 if (forced is None or not forced_as_draw) else (2 if forced_as_draw == "all" else 1)
        capi.check(self.lib.mtts_set_forced_mode(self._h, mode))
        out = np.zeros((R, cap, 8), dtype=np.int64)
        out_len = C.c_int32(0)
        scfg = sampler_cfgs(layers, do_samples)
        self._set_floors_and_bans(layers, do_samples)
        self.set_output_scores(output_scores)
        self.set_top_logprobs(top_logprobs)
        self._set_row_ids(row_ids, R)       # Philox row id of each row (default: its position in this batch)
        self._set_takes(takes)
        self._set_row_adapters(row_adapters, B)
        fptr, flen, dptr, dec = None, 0, None, None
        if forced is not None:
            forced = np.ascontiguousarray(forced, dtype=np.int64)
            flen = forced.shape[1]
            fptr = forced.ctypes.data
            dec = np.zeros((cap, B, 8), dtype=np.int64)
            dptr = dec.ctypes.data
        capi.check(self.lib.mtts_generate(self._h, ids.ctypes.data, m.ctypes.data, B, T, int(max_length), scfg,
                                          C.c_uint64(seed), out.ctypes.data, cap, C.byref(out_len), fptr, flen, dptr, None))
        res = out[:, :out_len.value].copy()
        ret = (res,) if forced is None else (res, dec[:out_len.value - (T - 7)].copy())
        if output_scores:
            ret += (np.ascontiguousarray(self.read_scores(out_len.value - (T - 7)).transpose(1, 0, 2)),)
        if top_logprobs:
            ret += (tuple(np.ascontiguousarray(np.swapaxes(a, 0, 1)) for a in self.read_top_logprobs(out_len.value - (T - 7))),)
        return ret if len(ret) > 1 else ret[0]

    def score(self, input_ids, attention_mask, labels=None, top_k=0):
        """Teacher-forced scoring (include/mtts.h: mtts_score): int64 [B,T,8] ids and labels (-100 = ignore), mask [B,T]
        right-padded or unpadded -> float32 [B,T,8], logp[b,t,c] = log_softmax(logits_c(h[b,t-1]))[labels[b,t,c]], NaN at
        t = 0, at ignored labels and at padding.  No run may be open; the engine's KV pool is as before afterwards.

        top_k > 0 (mtts_score_topk, 1..16): -> (logp, or None without labels; top_ids int32 [B,T,8,k]; top_logp float32
        [B,T,8,k]): the k most probable tokens of the same distributions, descending logit and ascending id among equals,
        whatever the label; -1 / NaN at t = 0 and at padding.  top_logp[..., j] has the bits logp would have for the label
        top_ids[..., j]."""
        ids, m = self._host_inputs(input_ids, attention_mask)
        B, T, _ = ids.shape
        lab = out = None
        if labels is not None:
            lab = np.ascontiguousarray(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels), dtype=np.int64)
            assert lab.shape == ids.shape
            out = np.empty((B, T, 8), dtype=np.float32)
        if not top_k:
            if lab is None:
                raise ValueError("score() needs labels, top_k > 0, or both")
            capi.check(self.lib.mtts_score(self._h, ids.ctypes.data, m.ctypes.data, lab.ctypes.data, B, T, out.ctypes.data, None))
            return out
        k = int(top_k)
        kk = max(k, 0)                                      # (a k the library refuses still gets buffers of a sane size)
        top_ids, top_logp = np.empty((B, T, 8, kk), dtype=np.int32), np.empty((B, T, 8, kk), dtype=np.float32)
        capi.check(self.lib.mtts_score_topk(self._h, ids.ctypes.data, m.ctypes.data, None if lab is None else lab.ctypes.data, B, T,
                                            None if out is None else out.ctypes.data, k, top_ids.ctypes.data, top_logp.ctypes.data, None))
        return out, top_ids, top_logp

    def begin(self, input_ids, attention_mask, max_length, layers=None, do_samples=None, seed=0, row_ids=None, takes=1,
              output_scores=False, row_adapters=None, top_logprobs=0):
        """Prefill; takes and row_adapters as in generate() (the run then has B*takes rows); output_scores: keep
        log-probabilities for read_scores(); top_logprobs=k: keep the raw distribution's for read_top_logprobs()."""
        ids, m = self._host_inputs(input_ids, attention_mask)
        B, T, _ = ids.shape
        self._B, self._T = B * int(takes), T
        self._set_floors_and_bans(layers, do_samples)
        self.set_output_scores(output_scores)
        self.set_top_logprobs(top_logprobs)
        self._set_row_ids(row_ids, B * int(takes))
        self._set_takes(takes)
        self._set_row_adapters(row_adapters, B)
        capi.check(self.lib.mtts_begin(self._h, ids.ctypes.data, m.ctypes.data, B, T, int(max_length),
                                       sampler_cfgs(layers, do_samples), C.c_uint64(seed), None))

    def step(self, n=1, stream=None):
        """Issue n decode steps on `stream` (torch.cuda.Stream; default: the device's default stream)."""
        capi.check(self.lib.mtts_step(self._h, int(n), C.c_void_p(stream.cuda_stream) if stream is not None else None))

    # ---- the split step: the caller between the heads and the sampler (include/mtts.h: mtts_step_begin) --------------
    def _split_buffers(self):
        """The score rows of a split step, allocated by torch once per run shape and padded as the logits are."""
        V0p, Vsp = (self.cfg["vocab_size"] + 31) // 32 * 32, (self.cfg["speech_vocab_size"] + 31) // 32 * 32
        bufs = getattr(self, "_split", None)
        if bufs is None or bufs[0].shape != (self._B, V0p) or bufs[1].shape != (self._B, 7, Vsp):
            bufs = (torch.full((self._B, V0p), float("-inf"), dtype=torch.float32, device=self.device),
                    torch.full((self._B, 7, Vsp), float("-inf"), dtype=torch.float32, device=self.device),
                    torch.zeros((self._B, 8), dtype=torch.int64, device=self.device))
            torch.cuda.synchronize(self.device)
            self._split = bufs
        return bufs

    def step_begin(self, stream=None, want_rows=True):
        """The first half of one decode step of a run started with begin(): everything in front of the sampler.
        -> (scores0 float32 [B, vocab_size], scores17 float32 [B, 7, speech_vocab_size], rows): CUDA views of buffers that
        live as long as the run's shape, holding for every (row, channel) the sampler evaluates this step the scores HF's
        built-in processors leave -- the reference's two masks, the run's bans and sequence rules, the repetition penalty;
        no temperature.  Edit them in place (on `stream`, or synchronise yourself): step_sample() samples from what they
        hold.  rows: bool [B], the rows evaluated (finished rows that cannot come back are skipped: their score rows are
        stale and ignored); want_rows=False: None, and no device synchronisation."""
        s0, s17, _ = self._split_buffers()
        rows = None
        if want_rows:
            st = self.slot_states()
            rows = (st[:, 0] != 0) & ((st[:, 1] != 0) | (st[:, 0] == 2))
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
        capi.check(self.lib.mtts_step_begin(self._h, s0.data_ptr(), s17.data_ptr(), sp))
        return s0[:, :self.cfg["vocab_size"]], s17[:, :, :self.cfg["speech_vocab_size"]], rows

    def step_sample(self, stream=None):
        """Between step_begin() and step_finish(): the sampler on the score rows as they stand (temperature, the warpers, argmax
        or the Philox draw; a row of -inf gives token 0 with a NaN score) and the state machine.  -> int64 [B, 8] CUDA tensor,
        the tokens the step appended (padding and flushes included); overwritten by the next step_sample()."""
        toks = self._split_buffers()[2]
        capi.check(self.lib.mtts_step_sample(self._h, toks.data_ptr(), C.c_void_p(stream.cuda_stream) if stream is not None else None))
        return toks

    def step_finish(self, stop=None, stream=None):
        """The rest of the step: `stop` (bool [B] or None) finishes rows as a stopping criterion of the reference does
        (modeling_asteroid.py:166-168: a row inside its EOS flush finishes the flush first; a stopped row emits
        (eos, speech_pad x 7) from the next step on), then the KV page bookkeeping and the forward pass.  Runs step_sample()
        itself when the caller did not."""
        m = None
        if stop is not None:
            m = np.ascontiguousarray(np.asarray(stop.cpu() if torch.is_tensor(stop) else stop).astype(bool).astype(np.uint8))
            if m.shape != (self._B,):
                raise ValueError(f"stop has shape {m.shape}, the run has {self._B} rows")
        capi.check(self.lib.mtts_step_finish(self._h, None if m is None else m.ctypes.data,
                                             C.c_void_p(stream.cuda_stream) if stream is not None else None))

    def sync_state(self, stream=None):
        s, d = C.c_int32(0), C.c_int32(0)
        capi.check(self.lib.mtts_sync_state(self._h, C.byref(s), C.byref(d),
                                            C.c_void_p(stream.cuda_stream) if stream is not None else None))
        return s.value, bool(d.value)

    def read_generated(self, capacity_steps):
        buf = np.zeros((capacity_steps, self._B, 8), dtype=np.int64)
        n = C.c_int32(0)
        capi.check(self.lib.mtts_read_generated(self._h, buf.ctypes.data, capacity_steps, C.byref(n)))
        return buf[:n.value]

    def read_scores(self, capacity_steps):
        """-> float32 [steps, rows, 8] log-probabilities of the run's generated rows (row space of read_generated)."""
        buf = np.zeros((max(int(capacity_steps), 1), self._B, 8), dtype=np.float32)
        n = C.c_int32(0)
        capi.check(self.lib.mtts_read_scores(self._h, buf.ctypes.data, buf.shape[0], C.byref(n)))
        return buf[:n.value]

    def read_top_logprobs(self, capacity_steps):
        """-> (logprobs float32 [steps, rows, 8], top_ids int32 [steps, rows, 8, k], top_logprobs float32 [steps, rows, 8, k])
        of the run's generated rows (row space of read_generated); k is the run's."""
        cap, k = max(int(capacity_steps), 1), max(self._topk, 1)
        lp = np.zeros((cap, self._B, 8), dtype=np.float32)
        ids = np.zeros((cap, self._B, 8, k), dtype=np.int32)
        tlp = np.zeros((cap, self._B, 8, k), dtype=np.float32)
        n = C.c_int32(0)
        capi.check(self.lib.mtts_read_top_logprobs(self._h, lp.ctypes.data, ids.ctypes.data, tlp.ctypes.data, cap, C.byref(n)))
        return lp[:n.value], ids[:n.value], tlp[:n.value]

    def read_logits(self):
        V0, Vs = self.cfg["vocab_size"], self.cfg["speech_vocab_size"]
        if self.dtype != "bf16":
            l0 = np.zeros((self._B, V0), dtype=np.float32)
            l17 = np.zeros((7, self._B, Vs), dtype=np.float32)
            capi.check(self.lib.mtts_read_logits_f32(self._h, l0.ctypes.data, l17.ctypes.data, None))
            return l0, l17
        l0 = np.zeros((self._B, V0), dtype=np.uint16)
        l17 = np.zeros((7, self._B, Vs), dtype=np.uint16)
        capi.check(self.lib.mtts_read_logits(self._h, l0.ctypes.data, l17.ctypes.data, None))
        f = lambda u: (u.astype(np.uint32) << 16).view(np.float32)
        return f(l0), f(l17)

    # ---- continuous batching ---------------------------------------------------------
    def sched_open(self, slots, gen_cap, layers=None, do_samples=None, output_scores=False, top_logprobs=0):
        self._B = int(slots)
        self._set_floors_and_bans(layers, do_samples)
        self.set_output_scores(output_scores)
        self.set_top_logprobs(top_logprobs)
        capi.check(self.lib.mtts_sched_open(self._h, int(slots), int(gen_cap), sampler_cfgs(layers, do_samples), None))

    def submit(self, slot, ids, max_length, seed=0, row_id=0, adapter=None):
        """ids int64 [T,8]: one delay-shifted prompt without padding (what shifting_inputs returns).  The dialogue
        draws from the Philox stream (seed; step, row_id, channel).  adapter: bank index it runs with (None / -1: none);
        fork() gives a take its source's."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        assert ids.ndim == 2 and ids.shape[1] == 8
        if adapter is not None and int(adapter) >= 0:
            capi.check(self.lib.mtts_set_slot_adapter(self._h, int(slot), int(adapter)))
        capi.check(self.lib.mtts_slot_submit_row(self._h, int(slot), ids.ctypes.data, ids.shape[0], int(max_length),
                                                 C.c_uint64(seed), int(row_id), None))

    def fork(self, src, dst, seed=0, row_id=0):
        """Scheduler mode: a take of the dialogue just submitted to slot `src` in the empty slot `dst` (shared prompt
        pages), drawing from (seed; step, row_id, channel) -- the tokens of submit(dst, that prompt, ..., seed, row_id)."""
        capi.check(self.lib.mtts_slot_fork(self._h, int(src), int(dst), C.c_uint64(seed), int(row_id), None))

    def slot_states(self):
        """-> int32 [slots,4]: active, unfinished, rows generated, tokens cached."""
        st = np.zeros((self._B, 4), dtype=np.int32)
        capi.check(self.lib.mtts_slot_states(self._h, st.ctypes.data, None))
        return st

    def slot_read(self, slot, capacity):
        buf = np.zeros((int(capacity), 8), dtype=np.int64)
        n = C.c_int32(0)
        capi.check(self.lib.mtts_slot_read(self._h, int(slot), buf.ctypes.data, int(capacity), C.byref(n)))
        return buf[:n.value].copy()

    def slot_read_scores(self, slot, capacity):
        """-> float32 [steps, 8] log-probabilities of the slot's generated rows (like slot_read)."""
        buf = np.zeros((max(int(capacity), 1), 8), dtype=np.float32)
        n = C.c_int32(0)
        capi.check(self.lib.mtts_slot_read_scores(self._h, int(slot), buf.ctypes.data, buf.shape[0], C.byref(n)))
        return buf[:n.value].copy()

    def slot_read_top_logprobs(self, slot, capacity):
        """-> (logprobs float32 [steps, 8], top_ids int32 [steps, 8, k], top_logprobs float32 [steps, 8, k]) of the slot's
        generated rows (like slot_read_scores)."""
        cap, k = max(int(capacity), 1), max(self._topk, 1)
        lp = np.zeros((cap, 8), dtype=np.float32)
        ids = np.zeros((cap, 8, k), dtype=np.int32)
        tlp = np.zeros((cap, 8, k), dtype=np.float32)
        n = C.c_int32(0)
        capi.check(self.lib.mtts_slot_read_top_logprobs(self._h, int(slot), lp.ctypes.data, ids.ctypes.data, tlp.ctypes.data, cap,
                                                        C.byref(n)))
        return lp[:n.value].copy(), ids[:n.value].copy(), tlp[:n.value].copy()

    def evict(self, slot):
        """Scheduler mode: drop the dialogue in `slot` and return its KV pages (it is re-submitted later)."""
        capi.check(self.lib.mtts_slot_evict(self._h, int(slot), None))

    def kv_pool_state(self):
        """-> (pages in the pool, pages free, pages per page-table row)."""
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        capi.check(self.lib.mtts_kv_pool_state(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def page_table(self, max_batch):
        """-> (int32 [max_batch, pages per row] page table as the host tracks it, int32 [max_batch] pages owned)."""
        _, _, mp = self.kv_pool_state()
        t = np.zeros((int(max_batch), mp), dtype=np.int32)
        n = np.zeros(int(max_batch), dtype=np.int32)
        capi.check(self.lib.mtts_read_page_table(self._h, t.ctypes.data, n.ctypes.data))
        return t, n

    def device_page_table(self, max_batch):
        """The page table as the device holds it (verification hook) -> int32 [max_batch, pages per row]."""
        _, _, mp = self.kv_pool_state()
        t = np.zeros((int(max_batch), mp), dtype=np.int32)
        capi.check(self.lib.mtts_debug_read_device_page_table(self._h, t.ctypes.data, None))
        return t

    def seq_state(self):
        """-> (needs_additional_steps[B], unfinished[B], kv_len[B]) numpy int32."""
        a, u, k = (np.zeros(self._B, dtype=np.int32) for _ in range(3))
        capi.check(self.lib.mtts_read_seq_state(self._h, a.ctypes.data, u.ctypes.data, k.ctypes.data, None))
        return a, u, k

    def export_codes(self, first, n, stream=None):
        """Frames first..first+n-1 -> int64 [8,B,n] device tensor, enqueued on `stream` (torch.cuda.Stream or None)."""
        out = torch.empty(8, self._B, n, dtype=torch.int64, device=self.device)
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
        capi.check(self.lib.mtts_export_codes(self._h, int(first), int(n), out.data_ptr(), sp))
        return out

    def kv_pack_stats(self):
        """Sealed KV pages of the live dialogues -> dict(k_pages, k_unsealed, v_pages, v_unsealed, k_layers_on, v_layers_on)
        (page x kv head x layer counts; `unsealed` = a lane did not fit the 13-bit form, the page is read as bf16;
        `*_layers_on` = layers whose reads currently take the sealed pages)."""
        o = np.zeros(6, dtype=np.int64)
        capi.check(self.lib.mtts_debug_kv_pack_stats(self._h, o.ctypes.data))
        return dict(zip(("k_pages", "k_unsealed", "v_pages", "v_unsealed", "k_layers_on", "v_layers_on"), (int(x) for x in o)))

    def step_plan(self, pages_bound):
        """How the decode step the engine would run now at `pages_bound` KV pages chooses its kernels (csrc/stepplan.h:
        describe) -> its lines, one per distinct launch group in issue order."""
        buf = C.create_string_buffer(4096)
        capi.check(self.lib.mtts_debug_step_plan(self._h, int(pages_bound), buf, len(buf)))
        return buf.value.decode().splitlines()

    def wseal_stats(self):
        """Sealed weight streams -> {kind: dict(groups, unsealed, on)} for gate_up, down, head0, heads17 (groups of 16 or 12
        k-tiles x lanes; `unsealed` = a lane did not fit the 13-bit form, that wave reads its bf16 tiles; `on` = the decode
        GEMMs of the kind read the sealed twin).  All tensors must be bound."""
        o = np.zeros(12, dtype=np.int64)
        capi.check(self.lib.mtts_debug_wseal_stats(self._h, o.ctypes.data))
        return {k: dict(groups=int(o[3 * i]), unsealed=int(o[3 * i + 1]), on=bool(o[3 * i + 2]))
                for i, k in enumerate(("gate_up", "down", "head0", "heads17"))}

    def debug_set_kv_len(self, n):
        capi.check(self.lib.mtts_debug_set_kv_len(self._h, int(n)))

    def attn_bench(self, phase, iters=112):
        """-> (avg ms per launch, algorithmic bytes per launch) of attention pass `phase` (1 scores, 2 PV, 3 combine,
        0 the three in a row, 4 the whole-row kernel) at the current decode state, measured over a train of
        back-to-back launches."""
        ms, by = C.c_float(0), C.c_int64(0)
        capi.check(self.lib.mtts_k_attn_bench(self._h, int(phase), int(iters), C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def profile(self, on=True):
        capi.check(self.lib.mtts_profile_enable(self._h, 1 if on else 0))

    def profile_read(self, which):
        ms, n, by = C.c_double(0), C.c_int64(0), C.c_int64(0)
        capi.check(self.lib.mtts_profile_read(self._h, which, C.byref(ms), C.byref(n), C.byref(by)))
        return ms.value, n.value, by.value
