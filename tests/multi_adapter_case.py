"""The case the multi-adapter test files and tools/multi_adapter_parity.py share: the tiny model, the adapter construction
of tests/test_adapter_gpu.py::_adapter, and the run that compares the unmerged row with the merged adapter."""
import functools

import numpy as np

from mtts import adapters, synth

CFG = synth.tiny()
NL = CFG["num_hidden_layers"]
RANK, ALPHA = 8, 16
SCALING = float(np.float32(ALPHA / np.sqrt(RANK)))          # rsLoRA: 5.657, not a power of two
PARITY_STEPS = 48
PARITY_GATE = 0.008              # tests/test_engine_gpu.py: MARGIN_OK, two bf16 ulps of relative top-2 gap
PARITY_PROMPT = (40, 31)         # real tokens, seed


def name(layer, proj):
    return f"model.language_model.layers.{layer}.{proj}.weight"


@functools.lru_cache(maxsize=None)
def adapter(which):
    """All seven modules of both layers, entries large enough to move the greedy ids (B A * scaling has about twice the
    base weights' standard deviation).  which "zero": lora_B all zero (PEFT's initial state)."""
    rng = np.random.default_rng(40 + (0 if which == "zero" else which))
    out = {}
    for n in range(NL):
        for p in adapters.PROJECTIONS:
            o, i = adapters.projection_shape(CFG, p)
            A, B = (rng.standard_normal((RANK, i)) * 0.1).astype(np.float32), (rng.standard_normal((o, RANK)) * 0.1).astype(np.float32)
            out[name(n, p)] = (A, np.zeros_like(B) if which == "zero" else B)
    return out


@functools.lru_cache(maxsize=None)
def weights():
    # speech rows of channel 0 boosted far enough that no dialogue leaves the speech range (and flushes) inside a test's
    # steps, with or without an adapter: the adapters change the hidden state, not the heads
    return synth.synth_weights(CFG, 11, bf16=True, emb_row_sigma=0.5, speech_boost=8.0)


def merged_weights(which):
    w = dict(weights())
    for nm, (A, B) in adapter(which).items():
        w[nm] = adapters.merge_spec(w[nm], A, B, SCALING, "bf16")
    return w


def prompts(lens, seed):
    """Left-padded batch whose row b holds exactly lens[b] real tokens (half text, half audio), delay-shifted."""
    rng = np.random.default_rng(seed)
    seqs = []
    for n in lens:
        raw = np.full((n, 8), 1024, dtype=np.int64)
        na = n // 2
        raw[:n - na, 0] = rng.integers(0, 151643, n - na)
        raw[n - na:, 0] = 151665 + rng.integers(0, 1024, na)
        raw[n - na:, 1:] = rng.integers(0, 1024, (na, 7))
        seqs.append(synth.shifting_inputs(raw, CFG["pad_token_id"]))
    return synth.left_pad(seqs, CFG["pad_token_id"])


def free_decisions(steps):
    """[steps, 1, 8] bool: the slots that are the model's decisions (channel c of step s < 7 is teacher-forced for c > s)."""
    free = np.ones((steps, 1, 8), dtype=bool)
    for s in range(min(7, steps)):
        free[s, :, s + 1:] = False
    return free


def engine(bank=True, **kw):
    """A bf16 engine on the tiny model.  bank: adapter 0 = adapter(1), 1 = adapter(2), 2 = the zero-B adapter."""
    from mtts.engine import Engine
    kw.setdefault("max_batch", 4)
    kw.setdefault("max_seq_len", 512)
    eng = Engine(CFG, **kw)
    eng.bind_state_dict(weights())
    if bank:
        for i, which in enumerate((1, 2, "zero")):
            eng.load_bank_adapter(i, adapter(which), SCALING)
    return eng


def margins_of(l0, l17, s):
    """Relative and absolute top-2 gap per channel of the decision of step s from its logits (oracle/asteroid_oracle.py:
    last_margins), with the loop's hard masks: 152694 on channel 0 while the prompt's delayed tail is fed, 1024 on a free
    speech channel."""
    out, gap = np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.float32)
    for c in range(8):
        sc = (l0 if c == 0 else l17[c - 1]).astype(np.float32).copy()
        if c == 0 and s < 7:
            sc[152694] = -np.inf
        if c and c <= s:
            sc[1024] = -np.inf
        top2 = np.partition(sc, -2)[-2:]
        out[c] = (top2[1] - top2[0]) / max(abs(top2[1]), 1e-6)
        gap[c] = top2[1] - top2[0]
    return out, gap


def merged_vs_unmerged():
    """48 greedy steps with adapter 1 MERGED (Engine.bind_lora, what load_adapter(a) does), replayed through the unmerged
    row.  -> dict(gen, dec [steps,1,8] the unmerged row's own decisions, margins and gaps [steps,1,8] of the merged run
    (relative and absolute top-2 gap), logit_diff [steps]: the largest |logit difference| of every step under the replay)."""
    ids, mask = prompts(PARITY_PROMPT[:1], PARITY_PROMPT[1])
    T, steps = ids.shape[1], PARITY_STEPS
    merged, bank = engine(False, max_batch=1), engine(True, max_batch=1)
    try:
        for nm, (A, B) in adapter(1).items():
            merged.bind_lora(nm, weights()[nm], A, B, SCALING)
        merged.begin(ids, mask, T + steps + 20)
        logits, margins, gaps = [], np.zeros((steps, 1, 8), np.float32), np.zeros((steps, 1, 8), np.float32)
        for s in range(steps):
            l0, l17 = merged.read_logits()
            logits.append((l0[0].copy(), l17[:, 0].copy()))
            margins[s, 0], gaps[s, 0] = margins_of(l0[0], l17[:, 0], s)
            merged.step(1)
            merged.sync_state()
        gen = merged.read_generated(steps)
        assert gen.shape[0] == steps
        merged.sched_open(1, 64)
        gold = np.concatenate([ids[:, :T - 7], gen.transpose(1, 0, 2)], axis=1)
        _, dec = bank.generate(ids, mask, T + steps + 20, forced=gold, row_adapters=[0])
        diffs = []
        for s in range(steps):                          # the unmerged row's logits for decision s: a replay of s forced tokens
            if s == 0:
                bank.begin(ids, mask, T + steps + 20, row_adapters=[0])
            else:
                bank.generate(ids, mask, T + steps + 20, forced=gold[:, :T - 7 + s], row_adapters=[0])
            u0, u17 = bank.read_logits()
            bank.sched_open(1, 64)
            diffs.append(max(float(np.abs(u0[0] - logits[s][0]).max()), float(np.abs(u17[:, 0] - logits[s][1]).max())))
        return dict(gen=gen, dec=dec, margins=margins, gaps=gaps, logit_diff=diffs)
    finally:
        merged.close()
        bank.close()
