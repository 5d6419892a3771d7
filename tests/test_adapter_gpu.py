"""LoRA adapters merged on the device (csrc/adapter.hip; mtts_k_lora_pack, mtts_bind_weight_lora, load_adapter).  -m gpu.

Every comparison is bitwise.  The merge is defined down to the order of its operations (mtts/adapters.py: merge_spec,
numpy float32), so the kernels have one right answer per element; and an engine that merged an adapter on the device
holds the same bytes as an engine that was bound with merge_spec's matrices, so everything it computes is equal too."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mtts import adapters, capi, synth  # noqa: E402

SENTINEL = 0xABCD


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bf16_bits(a):
    """float32 holding bf16 values -> their uint16 patterns."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def _place(buf, m16, cols, row_mul, row_off):
    """m16 uint16 [rows][cols] into the packed buffer: [n/32][k/16][lane = n%32 + 32*((k%16)/8)][8], n = s*row_mul + row_off."""
    KT = cols // 16
    n = (np.arange(m16.shape[0]) * row_mul + row_off)[:, None]
    k = np.arange(cols)[None, :]
    off = (((n // 32) * KT + k // 16) * 64 + n % 32 + 32 * ((k % 16) // 8)) * 8 + k % 8
    buf[off] = m16


# ---- 1. the hook against numpy ----------------------------------------------------------------------------------------------
def _inputs(rows, cols, r, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "exact":      # multiples of 1/8 in [-1, 1]: every sum is exact in fp32 (tests/test_adapter_cpu.py)
        return tuple(rng.integers(-8, 9, sh).astype(np.float32) / 8 for sh in ((rows, cols), (r, cols), (rows, r))) + (0.25,)
    W = synth.round_bf16((rng.standard_normal((rows, cols)) * 0.05).astype(np.float32))
    A = (rng.standard_normal((r, cols)) * 0.1).astype(np.float32)
    B = (rng.standard_normal((rows, r)) * 0.1).astype(np.float32)
    return W, A, B, 2.7          # not a power of two: the scaling multiply rounds


def _hook(W, A, B, scaling, rows_pad, row_mul, row_off, dtype, out):
    base = torch.from_numpy(W).to(torch.bfloat16 if dtype == 0 else torch.float32).cuda()
    a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    capi.check(capi.lib().mtts_k_lora_pack(base.data_ptr(), W.shape[0], W.shape[1], a.data_ptr(), b.data_ptr(), A.shape[0],
                                           C.c_float(scaling), rows_pad, row_mul, row_off, dtype, out.data_ptr(), None))
    torch.cuda.synchronize()


# (rows, cols, rows_pad, [(row_mul, row_off) of each matrix that shares the buffer])
PLACEMENTS = {
    "padded_80x48": (80, 48, 96, [(1, 0)]),                        # o / down: padded to 32 rows; one partial column block
    "k_in_qkv_64x256": (64, 256, 320, [(1, 128)]),                 # a k_proj inside q|k|v; two column blocks
    "gate_up_96x144": (96, 144, 192, [(2, 0), (2, 1)]),            # gate, then up, interleaved; a column tail
}


@pytest.mark.parametrize("kind", ["random", "exact"])
@pytest.mark.parametrize("r", [1, 16, 33, 256])
@pytest.mark.parametrize("place", list(PLACEMENTS))
def test_lora_pack_kernel_vs_numpy(place, r, kind):
    rows, cols, rows_pad, spots = PLACEMENTS[place]
    want = np.full(rows_pad * cols, SENTINEL, dtype=np.uint16)
    plain = want.copy()
    out = torch.from_numpy(want.view(np.int16).copy()).cuda()          # the 16-bit patterns; pre-filled with the sentinel
    out0 = out.clone()
    for i, (row_mul, row_off) in enumerate(spots):
        W, A, B, s = _inputs(rows, cols, r, kind, 100 * r + i)
        _hook(W, A, B, s, rows_pad, row_mul, row_off, 0, out)
        _hook(W, A, B, 0.0, rows_pad, row_mul, row_off, 0, out0)
        _place(want, _bf16_bits(adapters.merge_spec(W, A, B, s, "bf16")), cols, row_mul, row_off)
        _place(plain, _bf16_bits(W), cols, row_mul, row_off)
        # groups of the other matrices (gate before up is placed) and of the padding rows keep the sentinel: `want` holds it there
        assert (want == SENTINEL).sum() == (rows_pad - (i + 1) * rows) * cols          # (gate + up fill their buffer: 0 at the end)
        assert np.array_equal(out.cpu().numpy().view(np.uint16), want), i
        # the row-major forms of the fp32 / fp16 engines (their base holds values of the model dtype)
        for dtype, name in ((1, "fp32"), (2, "fp16")):
            Wd = W if name == "fp32" else W.astype(np.float16).astype(np.float32)
            rm = torch.full((rows, cols), 7.0, dtype=torch.float32, device="cuda")
            _hook(Wd, A, B, s, rows_pad, row_mul, row_off, dtype, rm)
            assert np.array_equal(_bits(rm.cpu().numpy()), _bits(adapters.merge_spec(Wd, A, B, s, name))), (name, i)
    assert np.array_equal(out0.cpu().numpy().view(np.uint16), plain)          # scaling 0: the plain pack of the base


def test_lora_pack_hook_argument_errors():
    t, o = (torch.zeros(64 * 64, dtype=torch.float32, device="cuda") for _ in range(2))
    call = lambda rows, cols, r, rows_pad, row_mul, row_off, dtype: capi.lib().mtts_k_lora_pack(
        t.data_ptr(), rows, cols, t.data_ptr(), t.data_ptr(), r, C.c_float(1.0), rows_pad, row_mul, row_off, dtype, o.data_ptr(), None)
    assert call(32, 32, 4, 32, 1, 0, 0) == 0
    for bad in ((32, 24, 4, 32, 1, 0, 0), (32, 32, 0, 32, 1, 0, 0), (32, 32, 257, 32, 1, 0, 0), (32, 32, 4, 32, 1, 1, 0),
                (32, 32, 4, 48, 1, 0, 0), (32, 32, 4, 32, 2, 0, 0), (32, 32, 4, 32, 1, 0, 3)):
        assert call(*bad) == capi.EINVAL, bad


# ---- 2. engines ---------------------------------------------------------------------------------------------------------------
CFG = synth.tiny()
NL = CFG["num_hidden_layers"]
RANK, ALPHA = 8, 16
SCALING = float(np.float32(ALPHA / np.sqrt(RANK)))          # rsLoRA: 5.657, not a power of two


def _name(layer, proj):
    return f"model.language_model.layers.{layer}.{proj}.weight"


@functools.lru_cache(maxsize=None)
def _adapter(which):
    """1: all seven modules of both layers, entries large enough to move the greedy ids (B A * scaling has about twice the
    base weights' standard deviation); 2: q_proj and v_proj of layer 1 only."""
    rng = np.random.default_rng(40 + which)
    targets = [(n, p) for n in range(NL) for p in adapters.PROJECTIONS] if which == 1 else [(1, "self_attn.q_proj"), (1, "self_attn.v_proj")]
    out = {}
    for n, p in targets:
        o, i = adapters.projection_shape(CFG, p)
        out[_name(n, p)] = ((rng.standard_normal((RANK, i)) * 0.1).astype(np.float32), (rng.standard_normal((o, RANK)) * 0.1).astype(np.float32))
    return out


@functools.lru_cache(maxsize=None)
def _weights(dtype):
    w = synth.synth_weights(CFG, 11, bf16=(dtype == "bf16"), emb_row_sigma=0.5, speech_boost=3.0)
    if dtype == "fp16":      # what Engine.bind makes of them: values of the model dtype
        w = {k: v.astype(np.float16).astype(np.float32) for k, v in w.items()}
    return w


def _merged(dtype, which):
    w = dict(_weights(dtype))
    for name, (A, B) in _adapter(which).items():
        w[name] = adapters.merge_spec(w[name], A, B, SCALING, dtype)
    return w


def _model(dtype, w):
    import modeling_asteroid as ma
    return ma.AsteroidTTSInstruct.from_state_dict(CFG, w, dtype=dtype).eval().to("cuda")


@functools.lru_cache(maxsize=None)
def _batch():
    ids, mask = synth.synth_prompts(CFG, 5, batch=2, prompt_len=24)
    rng = np.random.default_rng(6)
    sid = np.full((2, 20, 8), 1024, dtype=np.int64)             # scoring rows: unpadded, every label scored
    sid[:, :, 0] = rng.integers(0, 151643, (2, 20))
    sid[:, :, 1:] = rng.integers(0, 1024, (2, 20, 7))
    return ids, mask, sid, np.ones((2, 20), dtype=np.uint8)


def _run(eng):
    """Prefill logits, 12 greedy steps of ids and logits, score log-probabilities -> list of arrays."""
    ids, mask, sid, smask = _batch()
    eng.begin(ids, mask, ids.shape[1] + 40)
    out = list(eng.read_logits())
    for _ in range(12):
        eng.step(1)
        eng.sync_state()
        out += list(eng.read_logits())
    out.append(eng.read_generated(12).astype(np.float32))       # ids below 2^24: exact as fp32, compared as bits like the rest
    eng.sched_open(4, 64)                                       # ends the abandoned run (include/mtts.h: mtts_set_output_scores)
    out.append(eng.score(sid, smask, sid))
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _gen(model, ids, mask, new=12):
    return model.generate(torch.from_numpy(ids), torch.from_numpy(mask), max_new_tokens=new).numpy()


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp16"])
def test_engine_with_adapter_equals_engine_with_merged_weights(dtype):
    ids, mask, _, _ = _batch()
    m, m1, m2 = _model(dtype, _weights(dtype)), _model(dtype, _merged(dtype, 1)), _model(dtype, _merged(dtype, 2))
    try:
        # generate, load_adapter, generate again on one engine: the second run is the merged engine's (the captured steps were dropped)
        g_base = _gen(m, ids, mask)
        r_base = _run(m._engine)
        eng = m._engine
        m.load_adapter(_adapter(1), scaling=SCALING)
        assert m._engine is eng                                 # the resident engine, not a rebuild
        g1, want1 = _gen(m, ids, mask), _gen(m1, ids, mask)
        assert np.array_equal(g1, want1)
        assert g1.shape != g_base.shape or not np.array_equal(g1, g_base)
        r1, want_r1 = _run(m._engine), _run(m1._engine)
        assert _same(r1, want_r1)
        assert not np.array_equal(r1[-2], r_base[-2])           # the adapter moves the greedy ids within the 12 steps
        # adapter 1, then adapter 2: the bits of adapter 2 alone (the modules it does not target are back at their base)
        m.load_adapter(_adapter(2), scaling=SCALING)
        r2 = _run(m._engine)
        assert _same(r2, _run(m2._get_engine(2, 64))) and not _same(r2, r_base)
        # unload: the base engine's bits
        m.unload_adapter()
        assert _same(_run(m._engine), r_base)
        # a batch that makes _get_engine build a bigger engine: the adapter is applied to the new one
        m.load_adapter(_adapter(1), scaling=SCALING)
        wide, wmask = synth.synth_prompts(CFG, 9, batch=33, prompt_len=16)
        got = _gen(m, wide, wmask, new=4)
        assert m._engine is not eng and m._engine_key[2] == 64
        assert np.array_equal(got, _gen(m1, wide, wmask, new=4))
    finally:
        for x in (m, m1, m2):
            if x._engine is not None:
                x._engine.close()


def test_load_adapter_from_a_peft_directory(tmp_path):
    """The file path end to end: a checkpoint directory written here -> load_adapter(path) == load_adapter(tensors)."""
    import json
    import os
    from safetensors.torch import save_file
    ad = _adapter(2)
    os.makedirs(tmp_path / "checkpoint-10")
    with open(tmp_path / "checkpoint-10" / "adapter_config.json", "w") as f:
        json.dump(dict(peft_type="LORA", r=RANK, lora_alpha=ALPHA, use_rslora=True, bias="none"), f)
    save_file({f"base_model.model.{k[:-7]}.lora_{ab}.weight": torch.from_numpy(v) for k, pair in ad.items() for ab, v in zip("AB", pair)},
              str(tmp_path / "checkpoint-10" / "adapter_model.safetensors"))
    m, m2 = _model("bf16", _weights("bf16")), _model("bf16", _merged("bf16", 2))
    try:
        m.load_adapter(str(tmp_path / "checkpoint-10"))
        assert m._adapter[1] == SCALING
        ids, mask, _, _ = _batch()
        _gen(m, ids, mask, new=2), _gen(m2, ids, mask, new=2)   # builds the engines: the adapter comes after the weights
        assert _same(_run(m._engine), _run(m2._engine))
    finally:
        for x in (m, m2):
            if x._engine is not None:
                x._engine.close()


# ---- 3. state and arguments ---------------------------------------------------------------------------------------------------
def test_bind_weight_lora_state_and_argument_errors():
    from mtts.engine import Engine
    w = _weights("bf16")
    eng = Engine(CFG, max_batch=4, max_seq_len=256)
    try:
        eng.bind_state_dict(w)
        ids, mask, _, _ = _batch()
        name = _name(0, "self_attn.q_proj")
        A, B = _adapter(1)[name]
        base = torch.from_numpy(w[name]).to(torch.bfloat16).cuda()
        a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()

        def raw(nm=name, rows=base.shape[0], cols=base.shape[1], r=RANK):
            return eng.lib.mtts_bind_weight_lora(eng._h, nm.encode(), base.data_ptr(), rows, cols, a.data_ptr(), b.data_ptr(), r,
                                                 C.c_float(SCALING), None)

        eng.begin(ids, mask, ids.shape[1] + 40)
        eng.step(12)
        eng.sync_state()
        want = eng.read_generated(12)
        eng.sched_open(4, 64)
        # between begin and the end of a run: refused, and the weights are as they were
        eng.begin(ids, mask, ids.shape[1] + 40)
        eng.step(5)
        assert raw() == capi.ESTATE
        with pytest.raises(capi.MttsError) as ei:
            eng.bind_lora(name, w[name], A, B, SCALING)
        assert ei.value.code == capi.ESTATE
        eng.step(7)
        eng.sync_state()
        assert np.array_equal(eng.read_generated(12), want)
        eng.sched_open(4, 64)
        # arguments
        for nm in ("model.language_model.layers.0.input_layernorm.weight", "model.embedding_list.1.weight", "lm_heads.0.weight",
                   "model.language_model.norm.weight", "model.language_model.layers.0.self_attn.x_proj.weight", _name(NL, "self_attn.q_proj")):
            assert raw(nm=nm) == capi.EINVAL, nm
        assert raw(r=0) == capi.EINVAL and raw(r=257) == capi.EINVAL
        assert raw(rows=base.shape[0] - 32) == capi.EINVAL and raw(nm=_name(0, "self_attn.k_proj")) == capi.EINVAL
        with pytest.raises(ValueError):
            eng.bind_lora(name, w[name], A[:, :128], B, SCALING)
        # none of the refusals touched the weights; and the call itself works on this engine
        eng.begin(ids, mask, ids.shape[1] + 40)
        eng.step(12)
        eng.sync_state()
        assert np.array_equal(eng.read_generated(12), want)
        eng.sched_open(4, 64)
        assert raw() == 0
        torch.cuda.synchronize()
    finally:
        eng.close()
