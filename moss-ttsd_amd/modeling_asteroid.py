"""Drop-in for the reference's `modeling_asteroid` module on MI355X.

Keeps the call surface `generation_utils` / `inference.py` use
(reference modeling_asteroid.py: AsteroidTTSConfig :17-28, AsteroidTTSInstruct :288,
`.from_pretrained`, `.eval()`, `.to(device)`, `.generate(input_ids, attention_mask)`,
`.config`; and the labels branch of `forward`, :382-410), and routes everything that computes to libmtts.so (hand-written HIP for
gfx950) through mtts.engine.Engine.  There is no PyTorch forward here and no CPU path.
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import torch

from mtts import adapters, ban_spec, bias_spec, synth, topk_spec, warp_spec
from mtts.engine import Engine

_CFG_KEYS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
             "num_key_value_heads", "head_dim", "rms_norm_eps", "rope_theta", "max_position_embeddings",
             "channels", "speech_pad_token", "speech_vocab_size", "speech_token_range", "eos_token_id", "pad_token_id")


class AsteroidTTSConfig:
    """Qwen3Config fields + channels / speech_pad_token / speech_vocab_size / speech_token_range."""
    model_type = "asteroid_tts"

    def __init__(self, channels=8, speech_pad_token=1024, speech_vocab_size=1025, speech_token_range=(), **kw):
        base = synth.make_config()
        base.update(channels=channels, speech_pad_token=speech_pad_token, speech_vocab_size=speech_vocab_size)
        if speech_token_range:
            base["speech_token_range"] = list(speech_token_range)
        if "rope_parameters" in kw and isinstance(kw["rope_parameters"], dict):
            kw.setdefault("rope_theta", kw["rope_parameters"].get("rope_theta", base["rope_theta"]))
        if kw.get("head_dim") is None and "hidden_size" in kw and "num_attention_heads" in kw:
            kw["head_dim"] = kw["hidden_size"] // kw["num_attention_heads"]
        for k, v in kw.items():
            if k in base and v is not None:
                base[k] = v
        self.__dict__.update(base)
        self._extra = {k: v for k, v in kw.items() if k not in base}

    def to_dict(self):
        return {k: getattr(self, k) for k in _CFG_KEYS}

    @classmethod
    def from_pretrained(cls, path):
        with open(os.path.join(path, "config.json")) as f:
            return cls(**json.load(f))


class GenerationConfig:
    """The fields of generation_config.json the decode loop reads (modeling_asteroid.py:66-109)."""

    def __init__(self, **kw):
        self.max_new_tokens = kw.get("max_new_tokens")
        self.max_length = kw.get("max_length", 20)
        self.do_sample = bool(kw.get("do_sample", False))
        self.do_samples = kw.get("do_samples")
        self.layers = kw.get("layers")
        self.eos_token_id = kw.get("eos_token_id")
        self.temperature = kw.get("temperature")
        self.top_k = kw.get("top_k")
        self.top_p = kw.get("top_p")
        self.repetition_penalty = kw.get("repetition_penalty")
        # HF's probability floors (MinP / Epsilon / EtaLogitsWarper), which _get_logits_processor puts behind top-p
        self.min_p = kw.get("min_p")
        self.epsilon_cutoff = kw.get("epsilon_cutoff", 0.0)
        self.eta_cutoff = kw.get("eta_cutoff", 0.0)
        # HF's TypicalLogitsWarper (locally typical sampling), between min_p and epsilon_cutoff; HF's default 1.0 = none
        self.typical_p = kw.get("typical_p", 1.0)
        # HF's hard bans (NoRepeatNGram / SuppressTokens / MinNewTokensLength processors)
        self.no_repeat_ngram_size = kw.get("no_repeat_ngram_size", 0)
        self.suppress_tokens = kw.get("suppress_tokens")
        self.min_new_tokens = kw.get("min_new_tokens")
        # HF's SequenceBias / NoBadWords / MinLength / SuppressTokensAtBegin processors (mtts/bias_spec.py)
        self.sequence_bias = kw.get("sequence_bias")
        self.bad_words_ids = kw.get("bad_words_ids")
        self.min_length = kw.get("min_length", 0)
        self.begin_suppress_tokens = kw.get("begin_suppress_tokens")
        self.seed = kw.get("seed")
        self.num_return_sequences = kw.get("num_return_sequences", 1)

    @classmethod
    def from_pretrained(cls, path):
        p = os.path.join(path, "generation_config.json")
        if not os.path.exists(p):
            return cls()
        with open(p) as f:
            return cls(**json.load(f))

    def channel_settings(self, channels, **over):
        """-> (layers[8], do_samples[8]); the global-processor branch (:107-109) repeats one config.
        The probability floors min_p / epsilon_cutoff / eta_cutoff: in the global branch the top-level fields (or the
        `floors` keywords, generate()'s overrides for one call) join the one dict under the conditions on which HF's
        _get_logits_processor adds the warper: min_p is not None, 0 < epsilon_cutoff < 1, 0 < eta_cutoff < 1.  In the
        per-channel branch they come from layers[i] -- this engine's extension of the four keys the reference reads
        there -- and the top-level values are ignored, as that branch of the reference ignores every top-level warper.
        typical_p travels with them: HF adds its warper when typical_p is not None and < 1.0, so 1.0 (HF's default) and None
        leave the dict as it was.
        The hard bans no_repeat_ngram_size / suppress_tokens / min_new_tokens travel the same way, with two differences:
        they are processors, so in the global branch they join the dict whatever do_sample is (the reference's
        `[logits_processor] * channels` applies them on all eight channels), and HF's conditions are n not None and > 0,
        the list not None, m not None and > 0 with an eos_token_id.  A config that sets none gives the dicts it always gave.
        sequence_bias / bad_words_ids / min_length / begin_suppress_tokens (mtts/bias_spec.py) are processors too and travel
        like the bans.  HF's conditions: sequence_bias, bad_words_ids and begin_suppress_tokens not None, min_length not None
        and > 0 with an eos_token_id.  The lists of bad_words_ids equal to [eos_token_id] are dropped where the values are
        marshalled (mtts.engine.sampler_bias).  Forced BOS / EOS, prefix constraints, guidance and top_h are not read."""
        if self.do_samples is not None:
            layers = list(self.layers or [])
            layers += [{}] * (channels - len(layers))
            return layers, list(self.do_samples)
        one = {}
        if self.do_sample:
            one = dict(repetition_penalty=self.repetition_penalty, temperature=self.temperature,
                       top_k=self.top_k, top_p=self.top_p)
            for k in warp_spec.FLOOR_KEYS:
                v = over[k] if over.get(k) is not None else getattr(self, k)
                if v is not None and (k == "min_p" or 0.0 < float(v) < 1.0):
                    one[k] = v
            v = over["typical_p"] if over.get("typical_p") is not None else self.typical_p
            # (anything that is not 1.0 goes on and is refused where the values are checked)
            if v is not None and (isinstance(v, bool) or v != 1.0):
                one["typical_p"] = v
        elif self.repetition_penalty not in (None, 1.0):
            one = dict(repetition_penalty=self.repetition_penalty)
        ban = {k: (over[k] if over.get(k) is not None else getattr(self, k)) for k in ban_spec.BAN_KEYS}
        # (HF skips a size or count <= 0; anything that is no integer goes on and is refused where the values are checked)
        off = lambda v: v is None or (ban_spec.is_int(v) and v <= 0)
        if not off(ban["no_repeat_ngram_size"]):
            one["no_repeat_ngram_size"] = ban["no_repeat_ngram_size"]
        if ban["suppress_tokens"] is not None:
            one["suppress_tokens"] = ban["suppress_tokens"]
        if not off(ban["min_new_tokens"]) and self.eos_token_id is not None:
            one["min_new_tokens"] = ban["min_new_tokens"]
        bias = {k: (over[k] if over.get(k) is not None else getattr(self, k)) for k in bias_spec.BIAS_KEYS}
        for k in ("sequence_bias", "bad_words_ids", "begin_suppress_tokens"):
            if bias[k] is not None:
                one[k] = bias[k]
        if not off(bias["min_length"]) and self.eos_token_id is not None:
            one["min_length"] = bias["min_length"]
        return [one] * channels, [self.do_sample] * channels


def _load_safetensors_dir(path):
    from safetensors.torch import load_file
    files = sorted(glob.glob(os.path.join(path, "*.safetensors")))
    if not files:
        raise FileNotFoundError(f"no *.safetensors under {path}")
    sd = {}
    for f in files:
        sd.update(load_file(f))
    return sd


class GenerateOutput:
    """What generate(return_dict_in_generate=True) returns (HF GenerateDecoderOnlyOutput, modeling_asteroid.py:171-195
    of the reference), reduced to what the engine keeps: `sequences` and, with output_scores=True,
    `transition_scores` float32 [B*n, G, 8] = compute_transition_scores(sequences, scores, normalize_logits=True)
    per channel (NaN where the token is not a model decision) and `sequences_scores` [B*n] = their nansum.  The full
    per-step score rows are not materialised: `scores` is None.  With top_logprobs=k three more, the reduced form of
    output_logits (`logits` stays None): `logprobs` float32 [B*n, G, 8] = log_softmax(the step's raw logits, hard-coded
    masks only)[the sampler's decision], `top_ids` int64 [B*n, G, 8, k] and `top_logprobs` float32 [B*n, G, 8, k] = the k
    most probable tokens of that distribution, descending (ties by ascending id); NaN / -1 where transition_scores is NaN."""

    def __init__(self, sequences, transition_scores=None, logprobs=None, top_ids=None, top_logprobs=None):
        self.sequences = sequences
        self.scores = None
        self.logits = None
        self.transition_scores = transition_scores
        self.sequences_scores = None if transition_scores is None else torch.nansum(transition_scores, dim=(1, 2))
        self.logprobs = logprobs
        self.top_ids = top_ids
        self.top_logprobs = top_logprobs

    def __getitem__(self, k):
        return getattr(self, k)


class AsteroidTTSOutputWithPast:
    """The reference's output class (modeling_asteroid.py:30-37) as forward(labels=...) fills it with skip_logits: `loss`,
    `loss_all`, and None for everything the engine does not keep.  One field more: `token_logprobs` float32 [B,T,8], the
    log-probability of every label (NaN at t = 0, at ignored labels and at padding).  With forward(top_logprobs=k) two
    more: `top_ids` int64 [B,T,8,k] and `top_logprobs` float32 [B,T,8,k], the k most probable tokens of the distribution
    each slot is scored under, descending (ties by ascending id); -1 / NaN at t = 0 and at padding."""

    def __init__(self, loss=None, loss_all=None, token_logprobs=None, top_logprobs=None, top_ids=None):
        self.loss = loss
        self.loss_all = loss_all
        self.logits = self.logits_all = self.past_key_values = self.hidden_states = self.attentions = None
        self.token_logprobs = token_logprobs
        self.top_logprobs = top_logprobs
        self.top_ids = top_ids

    def __getitem__(self, k):
        return getattr(self, k)


class AsteroidTTSInstruct:
    MAX_ENGINE_BATCH = 128          # rows one engine pass carries (4 activation tiles share each weight stream)

    def __init__(self, config: AsteroidTTSConfig, state_dict=None, generation_config=None):
        self.config = config
        self.generation_config = generation_config or GenerationConfig(eos_token_id=config.eos_token_id)
        self.channels = config.channels
        self._sd = state_dict
        self._engine = None
        self._engine_key = None
        self.device = torch.device("cpu")
        self.training = False
        self.dtype = "bf16"             # "fp32": the strict-parity engine (from_pretrained(torch_dtype=torch.float32)); "fp16": its kernels with fp16 rounding points
        self.sample_seed = None         # explicit Philox key for the next generate() (tests); None = from torch's seed
        self.sample_rows = None         # Philox row id of each row of the next generate() (a rank's share of a sharded
                                        # batch sets its rows' job-wide positions); None = 0..B-1
        self._calls = 0
        self._adapter = None            # the active LoRA adapter: (tensors {weight name: (A, B)}, scaling); load_adapter()
        self._named = {}                # resident, unmerged adapters: name -> (bank index, tensors, scaling); load_adapter(adapter_name=)
        self.weights = [1 for _ in range(self.channels)]      # per-channel loss weights (modeling_asteroid.py:297)

    # ---- loading -----------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, model_path, torch_dtype=torch.bfloat16, attn_implementation=None, **_):
        if torch_dtype not in (torch.bfloat16, torch.float32, torch.float16, None):
            raise NotImplementedError("the MI355X engine is built for the three dtypes inference.py offers (bf16, fp16, fp32); "
                                      f"torch_dtype={torch_dtype} is not one of them")
        if not os.path.isdir(model_path):
            raise FileNotFoundError(f"{model_path}: local checkpoint directory required (no network here)")
        if adapters.is_adapter_dir(model_path):
            # a PEFT checkpoint (adapter_config.json + adapter_model.*, no model of its own): the base it names, then the adapter
            with open(os.path.join(model_path, "adapter_config.json")) as f:
                base = json.load(f).get("base_model_name_or_path")
            if not base or not os.path.isdir(base):
                raise FileNotFoundError(f"{model_path} is an adapter checkpoint and its base_model_name_or_path = {base!r} is not a "
                                        "local directory: load the base with from_pretrained(<local copy>) and call "
                                        "load_adapter(<this directory>)")
            m = cls.from_pretrained(base, torch_dtype=torch_dtype, attn_implementation=attn_implementation)
            m.load_adapter(model_path)
            return m
        cfg = AsteroidTTSConfig.from_pretrained(model_path)
        m = cls(cfg, _load_safetensors_dir(model_path), GenerationConfig.from_pretrained(model_path))
        m.dtype = {torch.float32: "fp32", torch.float16: "fp16"}.get(torch_dtype, "bf16")
        return m

    @classmethod
    def from_state_dict(cls, cfg_dict, state_dict, generation_config=None, dtype="bf16"):
        m = cls(AsteroidTTSConfig(**cfg_dict), state_dict, generation_config)
        m.dtype = dtype
        return m

    def eval(self):
        self.training = False
        return self

    def to(self, device):
        self.device = torch.device(device)
        if self._adapter is not None:
            self._adapter = ({k: tuple(t.to(self.device) for t in ab) for k, ab in self._adapter[0].items()}, self._adapter[1])
        self._named = {nm: (i, {k: tuple(t.to(self.device) for t in ab) for k, ab in ts.items()}, sc) for nm, (i, ts, sc) in self._named.items()}
        return self

    def is_speech_token(self, tokens):
        lo, hi = self.config.speech_token_range
        return (tokens >= lo) & (tokens < hi)

    # ---- engine ------------------------------------------------------------------
    def _get_engine(self, batch, need_len):
        if self.device.type != "cuda":
            raise RuntimeError("AsteroidTTSInstruct on MI355X needs model.to('cuda'): the HIP engine has no CPU path")
        cap_len = max(4096, int(need_len)) + 64
        slots = 32 if batch <= 32 else (64 if batch <= 64 else self.MAX_ENGINE_BATCH)
        if self._engine is not None and self._engine_key[:2] == (str(self.device), cap_len) and self._engine_key[2] >= slots:
            return self._engine
        key = (str(self.device), cap_len, slots)
        if self._engine is None or self._engine_key != key:
            if self._engine is not None:
                self._engine.close()
            self._engine = Engine(self.config.to_dict(), max_batch=slots, max_seq_len=cap_len,
                                  device=str(self.device), dtype=self.dtype)
            self._engine.bind_state_dict(self._sd)
            self._engine_key = key
            if self._adapter is not None:
                self._apply_adapter(self._engine, ())
            for idx, tensors, scaling in self._named.values():
                self._engine.load_bank_adapter(idx, tensors, scaling)
        return self._engine

    # ---- LoRA adapters (PEFT merge_and_unload on the resident engine: mtts/adapters.py, csrc/adapter.hip) ----------
    def _apply_adapter(self, eng, previous):
        """The active adapter's targets are bound merged; a weight in `previous` (names the engine holds merged with an
        earlier adapter) that it does not target goes back to its base."""
        tensors, scaling = self._adapter if self._adapter is not None else ({}, 0.0)
        for name, (A, B) in tensors.items():
            eng.bind_lora(name, self._sd[name], A, B, scaling, sync=False)
        torch.cuda.synchronize(eng.device)
        for name in previous:
            if name not in tensors:
                v = self._sd[name]
                eng.bind(name, torch.from_numpy(v) if isinstance(v, np.ndarray) else v)

    def load_adapter(self, path_or_tensors, scaling=None, adapter_name=None):
        """Make a LoRA adapter the active one: a PEFT checkpoint directory (adapter_config.json + adapter_model.safetensors
        | .bin; mtts.adapters.read_peft_dir lists what is refused), or {weight name: (lora_A [r, in], lora_B [out, r])}
        with `scaling` (lora_alpha / r, or / sqrt(r) for rsLoRA).  One adapter is active at a time: loading replaces the
        active one, and a weight the new adapter does not target goes back to its base.  On a resident engine this is one
        merge-and-pack pass per targeted matrix; an engine built later gets the adapter after its weights.

        With `adapter_name` (PEFT: model.load_adapter(path, adapter_name=...)) the adapter is instead kept resident and
        UNMERGED under that name, next to up to 15 others, for generate(adapter_names=[...]) to pick per prompt.  The same
        files and tensors are accepted and refused; in addition the rank is at most 64 and the model bf16.  The bound
        weights -- base, or merged with the active adapter -- stay as they are, and a named adapter's delta adds to them."""
        if adapter_name is not None:
            return self._load_named(str(adapter_name), path_or_tensors, scaling)
        if isinstance(path_or_tensors, (str, os.PathLike)):
            tensors, file_scaling, _ = adapters.read_peft_dir(os.fspath(path_or_tensors), self.config)
            scaling = file_scaling if scaling is None else scaling
        else:
            if scaling is None:
                raise ValueError("load_adapter(tensors) needs scaling (lora_alpha / r, or lora_alpha / sqrt(r) with rsLoRA)")
            tensors = {k: tuple(torch.as_tensor(t).detach() for t in ab) for k, ab in dict(path_or_tensors).items()}
            adapters.check_tensors(tensors, self.config)
        # widened to fp32 once; kept where the model is, so that a swap on a resident engine uploads nothing
        tensors = {k: tuple(torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous() for t in ab)
                   for k, ab in tensors.items()}
        missing = [k for k in tensors if k not in self._sd]
        if missing:
            raise ValueError(f"adapter targets {missing[0]!r}, which the base state dict does not hold")
        old = self._adapter
        self._adapter = (tensors, float(np.float32(scaling)))
        if self._engine is not None:
            try:
                self._apply_adapter(self._engine, tuple(old[0]) if old is not None else ())
            except Exception:
                self._adapter = old         # (a run is open: the engine refused the first matrix and holds what it held)
                raise
        return self

    def _load_named(self, name, path_or_tensors, scaling):
        if name == adapters.BASE_ADAPTER:
            raise ValueError(f"adapter_name {name!r} is the name of the base model in generate(adapter_names=...)")
        if self.dtype != "bf16":
            raise ValueError(f"load_adapter(adapter_name=...): resident adapters exist on the bf16 engine only, this model is {self.dtype}; "
                             "without adapter_name the adapter is merged, which every dtype supports")
        if isinstance(path_or_tensors, (str, os.PathLike)):
            tensors, file_scaling, _ = adapters.read_peft_dir(os.fspath(path_or_tensors), self.config)
            scaling = file_scaling if scaling is None else scaling
        else:
            if scaling is None:
                raise ValueError("load_adapter(tensors) needs scaling (lora_alpha / r, or lora_alpha / sqrt(r) with rsLoRA)")
            tensors = {k: tuple(torch.as_tensor(t).detach() for t in ab) for k, ab in dict(path_or_tensors).items()}
            adapters.check_tensors(tensors, self.config)
        for k, (A, _) in tensors.items():
            if int(A.shape[0]) > adapters.MAX_BANK_RANK:
                raise ValueError(f"{k}: rank {int(A.shape[0])} is above {adapters.MAX_BANK_RANK}, the most a resident adapter may have "
                                 "(merge it instead: load_adapter without adapter_name)")
        used = {i for i, _, _ in self._named.values()}
        idx = self._named[name][0] if name in self._named else next((i for i in range(adapters.MAX_BANK_ADAPTERS) if i not in used), None)
        if idx is None:
            raise ValueError(f"{adapters.MAX_BANK_ADAPTERS} adapters are resident already ({', '.join(self._named)}): delete_adapter() one first")
        tensors = {k: tuple(torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous() for t in ab)
                   for k, ab in tensors.items()}
        scaling = float(np.float32(scaling))
        if self._engine is not None:
            self._engine.load_bank_adapter(idx, tensors, scaling)
        self._named[name] = (idx, tensors, scaling)
        return self

    def delete_adapter(self, name):
        """Drop the resident adapter `name` (load_adapter(adapter_name=...)); its memory on the engine is freed."""
        if name not in self._named:
            raise ValueError(f"no resident adapter {name!r} (have: {', '.join(self._named) or 'none'})")
        idx = self._named[name][0]
        if self._engine is not None:
            self._engine.clear_bank_adapter(idx)
        del self._named[name]
        return self

    def adapter_names(self):
        """Names of the resident adapters, in the order they were loaded."""
        return list(self._named)

    def _row_adapters(self, adapter_names, B):
        """generate(adapter_names=[...]) -> bank index per prompt (-1: base), or None; ValueError before any engine work."""
        if adapter_names is None:
            return None
        names = list(adapter_names)
        if len(names) != B:
            raise ValueError(f"adapter_names has {len(names)} entries for a batch of {B} prompts")
        if self.dtype != "bf16":
            raise ValueError(f"generate(adapter_names=...): resident adapters exist on the bf16 engine only, this model is {self.dtype}")
        out = []
        for nm in names:
            if nm is None or nm == adapters.BASE_ADAPTER:
                out.append(-1)
            elif nm in self._named:
                out.append(self._named[nm][0])
            else:
                raise ValueError(f"adapter_names: no resident adapter {nm!r} (have: {', '.join(self._named) or 'none'}; "
                                 f"{adapters.BASE_ADAPTER!r} or None for the base model)")
        return out

    def unload_adapter(self):
        """Back to the base model: the projections the active adapter targets are rebound from the base state dict."""
        previous = tuple(self._adapter[0]) if self._adapter is not None else ()
        self._adapter = None
        if self._engine is not None:
            self._apply_adapter(self._engine, previous)
        return self

    # ---- teacher-forced loss (the labels branch of the reference's forward, modeling_asteroid.py:382-410) ----------
    def set_weights(self, weights):
        self.weights = weights

    def _check_forward_args(self, input_ids, attention_mask, labels, top_logprobs=None):
        """-> numpy (ids int64 [B,T,8], mask uint8 [B,T], labels int64 [B,T,8] -- all -100 when the call has none, which
        top_logprobs allows); ValueError before any engine exists."""
        if labels is None and top_logprobs is None:
            raise ValueError("forward() without labels: the MI355X engine keeps no logits, so there is nothing to return; "
                             "use generate() to decode, or pass labels for the per-channel losses")
        if top_logprobs is not None:
            topk_spec.check_k(top_logprobs)
        if input_ids is None:
            raise ValueError("forward() needs input_ids (inputs_embeds is not supported)")
        as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        ids = as_np(input_ids)
        lab = np.full(ids.shape, -100, dtype=np.int64) if labels is None else as_np(labels)
        if ids.ndim != 3:
            raise ValueError(f"input_ids must be [batch, seq, channels], got shape {tuple(ids.shape)}")
        B, T, C = ids.shape
        if C != self.channels:
            raise ValueError(f"Expected {self.channels} channels, got {C}")
        if tuple(lab.shape) != tuple(ids.shape):
            raise ValueError(f"labels must be shaped like input_ids {tuple(ids.shape)}, got {tuple(lab.shape)}")
        msk = np.ones((B, T), dtype=np.uint8) if attention_mask is None else (as_np(attention_mask) > 0).astype(np.uint8)
        if msk.shape != (B, T):
            raise ValueError(f"attention_mask must be [batch, seq] = {(B, T)}, got {tuple(msk.shape)}")
        ids, lab = ids.astype(np.int64), lab.astype(np.int64)
        lens = msk.sum(1)
        for b in range(B):
            if not msk[b, :lens[b]].all():
                kind = "left-padded" if not msk[b, 0] else "not ones followed by zeros"
                raise ValueError(f"attention_mask of row {b} is {kind}: forward(labels=...) takes right-padded or unpadded "
                                 "rows (the reference's positions are arange(T) for every row)")
        if (lab[msk == 0] != -100).any():
            raise ValueError("labels must be -100 wherever attention_mask is 0")
        vocab = np.array([self.config.vocab_size] + [self.config.speech_vocab_size] * (C - 1))
        if (((lab < 0) | (lab >= vocab)) & (lab != -100)).any():
            raise ValueError("labels must be -100 or inside the channel's vocabulary")
        return np.ascontiguousarray(ids), np.ascontiguousarray(msk), np.ascontiguousarray(lab)

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, labels=None, return_dict=None, top_logprobs=None, **kw):
        """The training-branch forward of the reference, forward only: LongTensor [B,T,8] ids and labels (-100 = ignore),
        mask [B,T] right-padded or unpadded -> AsteroidTTSOutputWithPast with `loss_all` (float32 [8]: the causal-LM loss of
        each channel, mean over its labelled slots; NaN for a channel without one), `loss` (their mean under
        `self.weights`) and `token_logprobs` [B,T,8]; return_dict=False -> (loss, loss_all, None).  The heads and the
        log-softmax run fused on the device (csrc/score.hip); logits are never materialised, as with the reference's
        skip_logits.  A batch beyond MAX_ENGINE_BATCH is scored in slices whose sums and counts are combined.

        top_logprobs=k (1..16): the output also carries `top_ids` [B,T,8,k] (int64, -1 where empty) and `top_logprobs`
        [B,T,8,k] (float32, NaN where empty): the k most probable tokens at every slot t >= 1 of a row, labelled or not,
        selected in the epilogue of the same head GEMM; top_logprobs[..., j] is bit for bit the token_logprobs value the
        label top_ids[..., j] would get.  With it labels may be omitted: loss, loss_all and token_logprobs are then None."""
        # what would change the reference's result, or ask for what the engine does not keep, is refused, not dropped
        bad = [k for k in ("position_ids", "inputs_embeds", "past_key_values", "cache_position") if kw.get(k) is not None]
        bad += [k for k in ("output_attentions", "output_hidden_states", "use_cache") if kw.get(k)]
        if kw.get("skip_logits") is False:
            bad.append("skip_logits=False")
        if bad:
            raise ValueError(f"forward(labels=...) does not take {', '.join(bad)}: positions are arange(T) over right-padded rows, "
                             "and the engine keeps no logits, cache, attentions or hidden states")
        ids, msk, lab = self._check_forward_args(input_ids, attention_mask, labels, top_logprobs)
        B, T, C = ids.shape
        k = 0 if top_logprobs is None else int(top_logprobs)
        eng = self._get_engine(min(B, self.MAX_ENGINE_BATCH), T)
        dev = input_ids.device if torch.is_tensor(input_ids) else self.device
        top_ids, top_lp = np.empty((B, T, C, k), dtype=np.int64), np.empty((B, T, C, k), dtype=np.float32)
        if labels is None:                                   # top-k alone: the first label-free forward
            for b0 in range(0, B, self.MAX_ENGINE_BATCH):
                sl = slice(b0, b0 + self.MAX_ENGINE_BATCH)
                _, top_ids[sl], top_lp[sl] = eng.score(ids[sl], msk[sl], None, top_k=k)
            if return_dict is not None and not return_dict:
                return (None, None, None)
            return AsteroidTTSOutputWithPast(None, None, None, torch.from_numpy(top_lp).to(dev), torch.from_numpy(top_ids).to(dev))
        lp = np.empty((B, T, C), dtype=np.float32)
        sums, counts = np.zeros(C, dtype=np.float64), np.zeros(C, dtype=np.int64)
        for b0 in range(0, B, self.MAX_ENGINE_BATCH):
            sl = slice(b0, b0 + self.MAX_ENGINE_BATCH)
            if k:
                lp[sl], top_ids[sl], top_lp[sl] = eng.score(ids[sl], msk[sl], lab[sl], top_k=k)
                part = lp[sl]
            else:
                part = lp[sl] = eng.score(ids[sl], msk[sl], lab[sl])
            ok = ~np.isnan(part)
            sums += np.where(ok, part, 0).astype(np.float64).sum(axis=(0, 1))
            counts += ok.sum(axis=(0, 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            loss_all = torch.from_numpy((-(sums / counts)).astype(np.float32)).to(self.device)   # 0 / 0: NaN, as cross_entropy's mean
        total_weight = sum(self.weights)
        loss = 0
        for w, l in zip([w / total_weight for w in self.weights], loss_all):
            loss = loss + w * l
        if return_dict is not None and not return_dict:
            return (loss, loss_all, None)
        if k:
            return AsteroidTTSOutputWithPast(loss, loss_all, torch.from_numpy(lp).to(dev), torch.from_numpy(top_lp).to(dev),
                                             torch.from_numpy(top_ids).to(dev))
        return AsteroidTTSOutputWithPast(loss, loss_all, torch.from_numpy(lp).to(dev))

    __call__ = forward

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, max_new_tokens=None, max_length=None, seed=None,
                 num_return_sequences=None, return_dict_in_generate=False, output_scores=False, adapter_names=None,
                 top_logprobs=None, min_p=None, epsilon_cutoff=None, eta_cutoff=None, no_repeat_ngram_size=None,
                 suppress_tokens=None, min_new_tokens=None, typical_p=None, sequence_bias=None, bad_words_ids=None,
                 min_length=None, begin_suppress_tokens=None, logits_processor=None, stopping_criteria=None, streamer=None, **kw):
        """LongTensor[B,T,8], mask[B,T] -> LongTensor[B*n, T-7+G, 8] (generation_utils.py:406-409), n =
        num_return_sequences (keyword, else generation_config; HF: row b*n+j is take j of prompt b, as generate on the
        repeat-interleaved batch returns it).  The n takes of a prompt share its prefill and its complete KV pages.
        return_dict_in_generate=True -> GenerateOutput (.sequences = that tensor); with output_scores=True it carries
        the per-token log-probabilities from the device sampler (modeling_asteroid.py:69-80,171-195 of the reference
        return full score rows; see GenerateOutput).
        adapter_names (PEFT's mixed-batch inference): one name per PROMPT of a resident adapter (load_adapter(adapter_name=)),
        "__base__" or None for none; the prompt's takes run with it.  A row's tokens are those of the single-prompt call.
        top_logprobs=k (1..16, needs return_dict_in_generate=True): the output also carries `logprobs`, `top_ids` and
        `top_logprobs` (GenerateOutput), the model's own distribution at every decision, selected on the device in the
        decode step; it changes no token and no transition score.
        min_p / epsilon_cutoff / eta_cutoff (HF's generate keywords): override generation_config's for this call in the
        global branch; with generation_config.do_samples set the floors are per channel and belong in layers[i].
        typical_p (HF's generate keyword; mtts/warp_spec.py): the same; 1.0 runs without it.
        no_repeat_ngram_size / suppress_tokens / min_new_tokens (HF's generate keywords): the same for the hard bans, which
        act on greedy and sampled channels alike (mtts/ban_spec.py); refused with do_samples set, like the floors.
        sequence_bias / bad_words_ids / min_length / begin_suppress_tokens (HF's generate keywords; mtts/bias_spec.py): the
        same again -- an additive fp32 term on a token, always or behind a token sequence; multi-token bans; EOS kept out
        while the channel is shorter than min_length; ids banned at the first free step.  Refused with do_samples set.
        logits_processor / stopping_criteria / streamer (HF's generate keywords; the reference's _sample takes all three,
        modeling_asteroid.py:53-61): any of them runs the call as a host loop over the engine's split step (_generate_hooked),
        one round trip per step and no captured step graph.  Every processor is called as processor(input_ids[..., c],
        scores_c) on each of the eight channels, behind the built-in processors and in front of the temperature and the
        warpers -- HF's order; every criterion as criterion(input_ids[..., 0], None) after the step's tokens are appended;
        the streamer gets the prompt, then next_tokens[:, 0].cpu() per step, then end().  Refused: logits_processor with
        do_samples set (the reference's per-channel branch ignores the caller's list), more rows than MAX_ENGINE_BATCH, an
        entry that is not callable, a streamer without put / end."""
        processors, criteria = self._check_hooks(logits_processor, stopping_criteria, streamer)
        hooked = bool(processors or criteria or streamer is not None)
        over = {k: v for k, v in (("min_p", min_p), ("epsilon_cutoff", epsilon_cutoff), ("eta_cutoff", eta_cutoff)) if v is not None}
        for name, v in over.items():
            warp_spec.check_floor(name, v, "generate(): ")
        if typical_p is not None:
            warp_spec.check_typical(typical_p, "generate(): ")
            over["typical_p"] = typical_p
        bans = {k: v for k, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("suppress_tokens", suppress_tokens),
                                  ("min_new_tokens", min_new_tokens)) if v is not None}
        for name, v in bans.items():
            ban_spec.check_ban(name, v, "generate(): ")
        over.update(bans)
        bias = {k: v for k, v in (("sequence_bias", sequence_bias), ("bad_words_ids", bad_words_ids), ("min_length", min_length),
                                  ("begin_suppress_tokens", begin_suppress_tokens)) if v is not None}
        for name, v in bias.items():
            bias_spec.check_bias(name, v, "generate(): ")
        over.update(bias)
        if over and self.generation_config.do_samples is not None:
            raise ValueError(f"generate({', '.join(over)}=...) with generation_config.do_samples set: the per-channel branch reads its "
                             "warpers and processors from generation_config.layers[i]; put the floors there")
        k = 0
        if top_logprobs is not None:
            k = topk_spec.check_k(top_logprobs)
            if not return_dict_in_generate:
                raise ValueError("top_logprobs needs return_dict_in_generate=True: a plain tensor of sequences cannot carry it")
        if return_dict_in_generate:
            bad = [k for k in ("output_logits", "output_attentions", "output_hidden_states") if kw.get(k)]
            if bad:
                raise ValueError(f"{', '.join(bad)} with return_dict_in_generate: the MI355X engine keeps no logits, attentions "
                                 "or hidden states; only output_scores (per-token log-probabilities) is available")
        want_lp = bool(return_dict_in_generate and output_scores)
        gc = self.generation_config
        B, T, C = input_ids.shape
        if C != self.channels:
            raise ValueError(f"Expected {self.channels} channels, got {C}")
        n = num_return_sequences if num_return_sequences is not None else getattr(gc, "num_return_sequences", 1)
        n = 1 if n is None else int(n)
        if n < 1:
            raise ValueError(f"num_return_sequences must be >= 1 (got {n})")
        if attention_mask is None:
            attention_mask = torch.ones(B, T)
        # HF: max_length = max_new_tokens + input length when max_new_tokens is given
        mnt = max_new_tokens if max_new_tokens is not None else gc.max_new_tokens
        if max_length is None:
            max_length = (T + mnt) if mnt is not None else gc.max_length
        layers, do_samples = gc.channel_settings(C, **over)
        for i, lc in enumerate(layers):
            warp_spec.floors_of(lc, f"generation_config, channel {i}: ")       # a bad value: ValueError before the device is touched
            warp_spec.typical_of(lc, f"generation_config, channel {i}: ")
            ban_spec.bans_of(lc, f"generation_config, channel {i}: ")
            bias_spec.bias_of(lc, f"generation_config, channel {i}: ")
        if n > 1 and not any(do_samples):
            # HF GenerationMixin: greedy search returns one sequence per prompt
            raise ValueError("Greedy methods (do_sample != True) without beam search do not support `num_return_sequences` "
                             f"different than 1 (got {n}).")
        if hooked and B * n > self.MAX_ENGINE_BATCH:
            raise ValueError(f"generate(logits_processor / stopping_criteria / streamer) with {B * n} rows: the hooks run on one static batch "
                             f"of at most {self.MAX_ENGINE_BATCH} rows (more go through the continuous batcher, whose steps are not split)")
        seed = self._next_seed(seed)
        ids = input_ids.detach().cpu().numpy()
        msk = attention_mask.detach().cpu().numpy()
        rows = list(range(B)) if self.sample_rows is None else [int(r) for r in self.sample_rows]
        if len(rows) != B:
            raise ValueError(f"sample_rows has {len(rows)} entries for a batch of {B}")
        row_adapters = self._row_adapters(adapter_names, B)
        R = B * n                       # take j of prompt b is row b*n+j and draws as row rows[b]*n+j of the expanded job
        # room for the reference's finished-row flushes past max_length: 14 steps at least, the whole chain
        # (6 * B + 8, include/mtts.h: mtts_generate) where that is cheap
        eng = self._get_engine(R, int(max_length) + 6 * min(R, self.MAX_ENGINE_BATCH) + 8)
        if hooked:
            out, lp, top = self._generate_hooked(eng, ids, msk, int(max_length), layers, do_samples, seed,
                                                 [r * n + j for r in rows for j in range(n)], n, want_lp, row_adapters, k,
                                                 processors, criteria, streamer, input_ids)
        elif R <= self.MAX_ENGINE_BATCH:
            # one static batch, the reference's semantics: finished rows emit (eos, 1024 x 7) until the batch ends
            out = eng.generate(ids, msk, int(max_length), layers=layers, do_samples=do_samples, seed=seed,
                               row_ids=[r * n + j for r in rows for j in range(n)], takes=n, output_scores=want_lp,
                               row_adapters=row_adapters, top_logprobs=k)
            out = out if isinstance(out, tuple) else (out,)
            out, lp, top = out[0], (out[1] if want_lp else None), (out[-1] if k else None)
        else:
            out, lp, top = self._generate_scheduled(eng, ids, msk, int(max_length), layers, do_samples, seed, rows, n, want_lp,
                                                    row_adapters, k)
        seq = torch.from_numpy(out).to(input_ids.device)
        if not return_dict_in_generate:
            return seq
        dev = input_ids.device
        go = GenerateOutput(seq, None if lp is None else torch.from_numpy(lp).to(dev))
        if top is not None:
            go.logprobs, go.top_logprobs = torch.from_numpy(top[0]).to(dev), torch.from_numpy(top[2]).to(dev)
            go.top_ids = torch.from_numpy(top[1].astype(np.int64)).to(dev)
        return go

    def _check_hooks(self, logits_processor, stopping_criteria, streamer):
        """generate()'s three hooks -> (processors, criteria) as lists; ValueError before any engine work.  None and an empty
        list are the same: nothing to call."""
        processors = [] if logits_processor is None else (list(logits_processor) if isinstance(logits_processor, (list, tuple)) or
                                                          not callable(logits_processor) else [logits_processor])
        criteria = [] if stopping_criteria is None else (list(stopping_criteria) if isinstance(stopping_criteria, (list, tuple)) or
                                                         not callable(stopping_criteria) else [stopping_criteria])
        for i, p in enumerate(processors):
            if not callable(p):
                raise ValueError(f"logits_processor[{i}] ({type(p).__name__}) is not callable: a processor is called as "
                                 "processor(input_ids, scores) -> scores")
        for i, c in enumerate(criteria):
            if not callable(c):
                raise ValueError(f"stopping_criteria[{i}] ({type(c).__name__}) is not callable: a criterion is called as "
                                 "criterion(input_ids, scores) -> bool per row")
        if streamer is not None and not (callable(getattr(streamer, "put", None)) and callable(getattr(streamer, "end", None))):
            raise ValueError(f"streamer ({type(streamer).__name__}) needs put(tokens) and end(), as transformers' BaseStreamer has them")
        if processors and self.generation_config.do_samples is not None:
            raise ValueError("generate(logits_processor=...) with generation_config.do_samples set: the reference's per-channel branch "
                             "builds its processors from generation_config.layers[i] and ignores the caller's list "
                             "(modeling_asteroid.py:95-106); unset do_samples to run the global branch")
        return processors, criteria

    def _generate_hooked(self, eng, ids, msk, max_length, layers, do_samples, seed, row_ids, takes, output_scores, row_adapters,
                         top_logprobs, processors, criteria, streamer, input_ids):
        """generate() with the caller's hooks: the reference's loop (modeling_asteroid.py:110-185) on the host, one split engine
        step per turn (mtts.engine.Engine.step_begin / step_sample / step_finish).  `input_ids` of the hooks is the reference's:
        the [rows, cur_len, 8] history on the device, left pads included, grown by each step's tokens.
        -> (sequences, lp or None, top or None) as Engine.generate returns them."""
        B, T, C = ids.shape
        base, R = T - 7, B * takes
        eng.begin(ids, msk, max_length, layers=layers, do_samples=do_samples, seed=seed, row_ids=row_ids, takes=takes,
                  output_scores=output_scores, row_adapters=row_adapters, top_logprobs=top_logprobs)
        try:
            if streamer is not None:
                streamer.put(input_ids.cpu() if torch.is_tensor(input_ids) else torch.from_numpy(ids))     # HF: the prompt first
            hist, cur, steps, done = None, base, 0, False
            while not done:
                s0, s17, _ = eng.step_begin(want_rows=False)
                if hist is None:                   # one buffer for the whole run; the hooks see views of its first cur slots
                    hist = torch.zeros((R, base + 64, C), dtype=torch.int64, device=s0.device)
                    hist[:, :base] = torch.from_numpy(np.repeat(ids[:, :base], takes, axis=0)).to(s0.device)
                for c in range(C if processors else 0):
                    view = s0 if c == 0 else s17[:, c - 1]
                    scores = view
                    for p in processors:
                        scores = p(hist[:, :cur, c], scores)
                    if scores is not view:
                        if not torch.is_tensor(scores) or tuple(scores.shape) != tuple(view.shape):
                            got = tuple(scores.shape) if torch.is_tensor(scores) else type(scores).__name__
                            raise ValueError(f"logits_processor returned {got} on channel {c}, expected a tensor of shape {tuple(view.shape)}")
                        view.copy_(scores)
                toks = eng.step_sample()
                if cur == hist.shape[1]:
                    hist = torch.cat([hist, torch.zeros_like(hist)], dim=1)
                hist[:, cur] = toks
                cur += 1
                if streamer is not None:           # in front of this step's stopping criteria, as in the reference (:161-168)
                    streamer.put(toks[:, 0].cpu())
                stop = None
                for crit in criteria:
                    r = torch.as_tensor(crit(hist[:, :cur, 0], None)).to(device=toks.device, dtype=torch.bool)
                    r = r.expand(R) if r.dim() == 0 else r.reshape(R)
                    stop = r if stop is None else (stop | r)
                eng.step_finish(stop)
                steps, done = eng.sync_state()
            if streamer is not None:
                streamer.end()
        except BaseException:
            try:        # the run is abandoned mid-flight: end it, so that the next one may start with other settings
                eng.sched_open(1, 8, output_scores=output_scores, top_logprobs=top_logprobs)
            except Exception:
                pass
            raise
        gen = eng.read_generated(steps)                                     # [steps, R, 8]
        out = np.concatenate([np.repeat(ids[:, :base], takes, axis=0), np.ascontiguousarray(gen.transpose(1, 0, 2))], axis=1)
        lp = np.ascontiguousarray(eng.read_scores(steps).transpose(1, 0, 2)) if output_scores else None
        top = tuple(np.ascontiguousarray(np.swapaxes(a, 0, 1)) for a in eng.read_top_logprobs(steps)) if top_logprobs else None
        return out, lp, top

    def _next_seed(self, seed):
        """Philox key of this call.  Explicit `seed=` / `generation_config.seed` / `model.sample_seed` win; otherwise it
        follows torch's global seed, which is what the reference's `inference.py --seed` sets through
        accelerate.set_seed (inference.py:69-72), advanced per call so that successive batches differ."""
        gc = self.generation_config
        if seed is None:
            seed = gc.seed if gc.seed is not None else self.sample_seed
        if seed is None:
            seed = (int(torch.initial_seed()) + 0x9E3779B97F4A7C15 * self._calls) & 0xFFFFFFFFFFFFFFFF
        self._calls += 1
        return int(seed)

    def _generate_scheduled(self, eng, ids, msk, max_length, layers, do_samples, seed, rows, takes=1, output_scores=False,
                            row_adapters=None, top_logprobs=0):
        """More rows than one pass carries: the continuous batcher serves them through MAX_ENGINE_BATCH slots (a
        finished dialogue's slot and KV pages go to the next one).  Row i draws from the Philox stream
        (seed; step, rows[i], channel) -- the stream row i of one static batch would use, so the same seed and prompts
        give the same tokens on either side of the 128-row limit (what differs: a dialogue cut off by max_length leaves
        at once here, while the reference keeps evaluating it and may resurrect it for a flush while another row is
        still flushing, modeling_asteroid.py:140-141,168).  -> (sequences, lp or None, (logprobs, top_ids, top_logprobs) or
        None), the per-row arrays padded with NaN / -1 behind each dialogue's own end."""
        from mtts.scheduler import ContinuousBatcher
        B, T, C = ids.shape
        base = T - 7
        pads = [int(np.argmax(msk[b, :base] > 0)) for b in range(B)]
        prompts = [ids[b, pads[b]:] for b in range(B)]
        new = max_length - T
        cb = ContinuousBatcher(eng, slots=self.MAX_ENGINE_BATCH, gen_cap=max_length - base + 8, layers=layers,   # max_new + 7 flush steps
                               do_samples=do_samples)
        res = cb.run(prompts, new, seeds=[seed] * B, row_ids=rows, takes=takes, output_scores=output_scores,
                     adapters=row_adapters, top_logprobs=top_logprobs or None)     # row k = take k % takes of prompt k // takes
        if top_logprobs:
            res, sc, tops = res
        else:
            (res, sc), tops = (res if output_scores else (res, None)), None
        G = max(r.shape[0] - (T - pads[k // takes] - 7) for k, r in enumerate(res))
        full = np.full((B * takes, base + G, C), self.config.speech_pad_token, dtype=np.int64)
        full[:, :, 0] = self.config.eos_token_id            # finished-row padding (modeling_asteroid.py:155-158)
        for k, r in enumerate(res):
            b = k // takes
            full[k, :base] = ids[b, :base]
            gen = r[T - pads[b] - 7:]
            full[k, base:base + gen.shape[0]] = gen
        lp = top = None
        if output_scores:
            lp = np.full((B * takes, G, C), np.nan, dtype=np.float32)      # NaN: padding after a dialogue has left
            for k, v in enumerate(sc):
                lp[k, :v.shape[0]] = v
        if top_logprobs:
            top = (np.full((B * takes, G, C), np.nan, dtype=np.float32), np.full((B * takes, G, C, top_logprobs), -1, dtype=np.int32),
                   np.full((B * takes, G, C, top_logprobs), np.nan, dtype=np.float32))
            for dst, src in zip(top, tops):
                for k, v in enumerate(src):
                    dst[k, :v.shape[0]] = v
        return full, lp, top
