"""mtts.adapters without a GPU: the PEFT checkpoint reader on directories this file writes itself, and merge_spec -- the
numpy float32 statement of the merge the device kernels are held to bit for bit (tests/test_adapter_gpu.py) -- against
float64, against torch's own in-place merge on the CPU, and on inputs whose sums are exact."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mtts import adapters, synth  # noqa: E402

CFG = synth.tiny()
L = CFG["num_hidden_layers"]


def _name(layer, proj):
    return f"model.language_model.layers.{layer}.{proj}.weight"


def _tensors(r=16, layers=None, projs=adapters.PROJECTIONS, seed=0):
    rng = np.random.default_rng(seed)
    out = {}
    for n in (range(L) if layers is None else layers):
        for p in projs:
            o, i = adapters.projection_shape(CFG, p)
            out[_name(n, p)] = (rng.standard_normal((r, i)).astype(np.float32) * 0.05, rng.standard_normal((o, r)).astype(np.float32) * 0.05)
    return out


def _write(path, tensors, fmt="safetensors", key=".lora_{}.weight", store=torch.float32, extra=None, **cfg):
    os.makedirs(path, exist_ok=True)
    config = dict(peft_type="LORA", r=16, lora_alpha=32, use_rslora=True, bias="none", fan_in_fan_out=False, use_dora=False,
                  modules_to_save=None, rank_pattern={}, alpha_pattern={}, base_model_name_or_path="fnlp/MOSS-TTSD-v0.5",
                  target_modules=["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"])
    config.update(cfg)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(config, f)
    sd = {}
    for name, (A, B) in tensors.items():
        mod = "base_model.model." + name[:-len(".weight")]
        sd[mod + key.format("A")] = torch.from_numpy(A).to(store)
        sd[mod + key.format("B")] = torch.from_numpy(B).to(store)
    sd.update(extra or {})
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(sd, os.path.join(path, "adapter_model.safetensors"))
    else:
        torch.save(sd, os.path.join(path, "adapter_model.bin"))
    return str(path)


# ---- the reader ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
@pytest.mark.parametrize("key", [".lora_{}.weight", ".lora_{}.default.weight"])
def test_reader_formats_and_key_forms(tmp_path, fmt, key):
    want = _tensors()
    got, scaling, config = adapters.read_peft_dir(_write(tmp_path / "ck", want, fmt=fmt, key=key), CFG)
    assert sorted(got) == sorted(want) and len(got) == 7 * L
    for k in want:
        for g, w in zip(got[k], want[k]):
            assert g.dtype == np.float32 and g.flags["C_CONTIGUOUS"] and np.array_equal(g, w)
    assert scaling == 8.0 and config["r"] == 16


def test_reader_scaling_rules(tmp_path):
    t = _tensors()
    assert adapters.read_peft_dir(_write(tmp_path / "rs", t, use_rslora=True), CFG)[1] == 8.0        # 32 / sqrt(16)
    assert adapters.read_peft_dir(_write(tmp_path / "plain", t, use_rslora=False), CFG)[1] == 2.0    # 32 / 16
    t5 = _tensors(r=5)
    s = adapters.read_peft_dir(_write(tmp_path / "r5", t5, r=5, lora_alpha=7, use_rslora=True), CFG)[1]
    assert s == float(np.float32(7 / np.sqrt(5)))                                                     # one fp32 value


def test_reader_widens_bf16_storage(tmp_path):
    want = _tensors()
    got = adapters.read_peft_dir(_write(tmp_path / "ck", want, store=torch.bfloat16), CFG)[0]
    for k in want:
        for g, w in zip(got[k], want[k]):
            assert g.dtype == np.float32 and np.array_equal(g, synth.round_bf16(w))


def test_reader_subsets(tmp_path):
    want = _tensors(layers=[1], projs=("self_attn.q_proj", "self_attn.v_proj"))
    got = adapters.read_peft_dir(_write(tmp_path / "ck", want), CFG)[0]
    assert sorted(got) == [_name(1, "self_attn.q_proj"), _name(1, "self_attn.v_proj")]
    # without a model config the file alone decides (shapes and the layer count are then the engine's to check)
    assert sorted(adapters.read_peft_dir(str(tmp_path / "ck"))[0]) == sorted(got)


@pytest.mark.parametrize("field,over", [
    ("peft_type", dict(peft_type="IA3")),
    ("use_dora", dict(use_dora=True)),
    ("bias", dict(bias="all")),
    ("fan_in_fan_out", dict(fan_in_fan_out=True)),
    ("modules_to_save", dict(modules_to_save=["lm_heads"])),
    ("rank_pattern", dict(rank_pattern={"q_proj": 8})),
    ("alpha_pattern", dict(alpha_pattern={"q_proj": 8})),
])
def test_reader_refuses_config_fields(tmp_path, field, over):
    with pytest.raises(ValueError, match=field):
        adapters.read_peft_dir(_write(tmp_path / "ck", _tensors(layers=[0]), **over), CFG)


def test_reader_refuses_tensors(tmp_path):
    r, H = 16, CFG["hidden_size"]
    ab = lambda o, i: (np.zeros((r, i), np.float32), np.zeros((o, r), np.float32))
    with pytest.raises(ValueError, match="lm_heads.0"):                                    # a target outside the seven
        adapters.read_peft_dir(_write(tmp_path / "a", {"lm_heads.0.weight": ab(1025, H)}), CFG)
    with pytest.raises(ValueError, match="input_layernorm"):
        adapters.read_peft_dir(_write(tmp_path / "b", {_name(0, "input_layernorm"): ab(H, H)}), CFG)
    with pytest.raises(ValueError, match=f"layer index {L}"):                              # a layer past the model's
        adapters.read_peft_dir(_write(tmp_path / "c", {_name(L, "self_attn.q_proj"): ab(*adapters.projection_shape(CFG, "self_attn.q_proj"))}), CFG)
    with pytest.raises(ValueError, match=r"\[512, 128\]"):                                 # the shape
        adapters.read_peft_dir(_write(tmp_path / "d", {_name(0, "self_attn.q_proj"): ab(512, 128)}), CFG)
    with pytest.raises(ValueError, match="r = 16"):                                        # the rank the config states
        adapters.read_peft_dir(_write(tmp_path / "e", _tensors(r=8, layers=[0])), CFG)
    one = _tensors(layers=[0], projs=("mlp.down_proj",))
    p = _write(tmp_path / "f", one, fmt="bin")
    sd = torch.load(os.path.join(p, "adapter_model.bin"), weights_only=True)
    del sd["base_model.model." + _name(0, "mlp.down_proj")[:-7] + ".lora_B.weight"]
    torch.save(sd, os.path.join(p, "adapter_model.bin"))
    with pytest.raises(ValueError, match="lora_A without lora_B"):
        adapters.read_peft_dir(p, CFG)
    with pytest.raises(ValueError, match="lora_magnitude_vector"):                         # nothing is dropped silently
        adapters.read_peft_dir(_write(tmp_path / "g", one, extra={"base_model.model.x.lora_magnitude_vector": torch.zeros(4)}), CFG)
    with pytest.raises(FileNotFoundError):
        os.makedirs(tmp_path / "h")
        with open(tmp_path / "h" / "adapter_config.json", "w") as f:
            json.dump(dict(peft_type="LORA", r=16, lora_alpha=32), f)
        adapters.read_peft_dir(str(tmp_path / "h"), CFG)


def test_from_pretrained_on_an_adapter_checkpoint_needs_a_local_base(tmp_path):
    import modeling_asteroid as ma
    p = _write(tmp_path / "checkpoint-10", _tensors(layers=[0]))
    assert adapters.is_adapter_dir(p)
    with pytest.raises(FileNotFoundError, match="base_model_name_or_path"):
        ma.AsteroidTTSInstruct.from_pretrained(p)


def test_load_adapter_before_an_engine_exists(tmp_path):
    """Loading needs no GPU: the adapter is kept for the engine that is built later; a bad one is refused at once."""
    import modeling_asteroid as ma
    w = {k: v for k, v in synth.synth_weights(CFG, 1).items()}
    m = ma.AsteroidTTSInstruct.from_state_dict(CFG, w)
    m.load_adapter(_write(tmp_path / "ck", _tensors(layers=[1])))
    assert len(m._adapter[0]) == 7 and m._adapter[1] == 8.0
    with pytest.raises(ValueError, match="scaling"):
        m.load_adapter(_tensors(layers=[0]))
    with pytest.raises(ValueError, match="layer index"):
        m.load_adapter({_name(L, "mlp.up_proj"): (np.zeros((4, 256), np.float32), np.zeros((512, 4), np.float32))}, scaling=1.0)
    assert len(m._adapter[0]) == 7                       # the refused ones changed nothing
    m.load_adapter(_tensors(r=4, layers=[0], projs=("mlp.up_proj",)), scaling=0.5)
    assert list(m._adapter[0]) == [_name(0, "mlp.up_proj")] and m._adapter[1] == 0.5
    assert m.unload_adapter()._adapter is None


# ---- merge_spec ------------------------------------------------------------------------------------------------------------
def _case(out=96, inn=80, r=16, seed=3, dtype="bf16"):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((out, inn)) * 0.05).astype(np.float32)
    W = {"bf16": synth.round_bf16, "fp16": lambda x: x.astype(np.float16).astype(np.float32), "fp32": lambda x: x}[dtype](W)
    A = (rng.standard_normal((r, inn)) * 0.1).astype(np.float32)
    B = (rng.standard_normal((out, r)) * 0.1).astype(np.float32)
    return W, A, B


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("r", [1, 16, 33, 256])
def test_merge_spec_vs_float64(dtype, r):
    """|merge_spec - exact| <= half an ulp of the result in the model dtype (its one rounding) + the fp32 error in front
    of it: r products, r - 1 additions that round (0 + x is exact), the scaling and the final add.  No term passes through
    more than r + 2 of these roundings, each of relative error 2^-24 on a partial result whose magnitude the sum of
    absolute values bounds: (r + 2) * 2^-24 * (|W| + |s| * sum_j |B_nj A_jk|), to first order."""
    W, A, B = _case(r=r, dtype=dtype)
    s = 8.0
    got = adapters.merge_spec(W, A, B, s, dtype).astype(np.float64)
    exact = W.astype(np.float64) + s * (B.astype(np.float64) @ A.astype(np.float64))
    mag = np.abs(W).astype(np.float64) + abs(s) * (np.abs(B).astype(np.float64) @ np.abs(A).astype(np.float64))
    # half an ulp of the result: the spacing of the model dtype at |got| (numpy's spacing for fp16 / fp32; 2^-7 of the
    # binade for bf16's 8 significant bits)
    if dtype == "bf16":
        half_ulp = 0.5 * 2.0 ** (np.floor(np.log2(np.maximum(np.abs(got), 2.0 ** -126))) - 7)
    elif dtype == "fp16":
        half_ulp = 0.5 * np.spacing(np.abs(got).astype(np.float16)).astype(np.float64)
    else:
        half_ulp = 0.5 * np.spacing(np.abs(got).astype(np.float32)).astype(np.float64)
    bound = half_ulp + (r + 2) * 2.0 ** -24 * mag
    err = np.abs(got - exact)
    print(f"{dtype} r={r}: max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("r", [1, 16, 33])
def test_merge_spec_equals_torch_inplace_merge(r):
    """PEFT's merge on a bf16 base: weight.data += delta with delta fp32.  With delta built in merge_spec's order, torch on
    the CPU gives the same bits (its bf16 += fp32 rounds once, from the fp32 sum)."""
    W, A, B = _case(r=r)
    s = float(np.float32(32 / np.sqrt(16)))
    tA, tB = torch.from_numpy(A), torch.from_numpy(B)
    acc = torch.zeros(W.shape, dtype=torch.float32)
    for j in range(r):
        acc = acc + tB[:, j:j + 1] * tA[j:j + 1, :]
    delta = acc * s
    w = torch.from_numpy(W).to(torch.bfloat16)
    w += delta
    got = adapters.merge_spec(W, A, B, s, "bf16")
    assert np.array_equal(w.float().numpy().view(np.uint32), got.view(np.uint32))
    # and it is not W + bf16(delta): the two differ somewhere on these inputs (r = 1 included)
    twice = (torch.from_numpy(W).to(torch.bfloat16) + delta.to(torch.bfloat16)).float().numpy()
    assert not np.array_equal(twice, got)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_merge_spec_exact_inputs(dtype):
    """Entries that are multiples of 1/8 in [-1, 1] and a power-of-two scaling: every product is a multiple of 1/64, every
    partial sum of r <= 256 of them is below 2^9 with 6 fractional bits, exact in fp32 in any order; so merge_spec is the
    model-dtype rounding of the exact value."""
    rng = np.random.default_rng(5)
    out, inn, r = 64, 48, 33
    W, A, B = (rng.integers(-8, 9, sh).astype(np.float32) / 8 for sh in ((out, inn), (r, inn), (out, r)))
    exact = W.astype(np.float64) + 0.25 * (B.astype(np.float64) @ A.astype(np.float64))
    assert np.array_equal(exact, exact.astype(np.float32))
    want = {"bf16": synth.round_bf16(exact.astype(np.float32)), "fp16": exact.astype(np.float16).astype(np.float32),
            "fp32": exact.astype(np.float32)}[dtype]
    assert np.array_equal(adapters.merge_spec(W, A, B, 0.25, dtype).view(np.uint32), want.view(np.uint32))


# ---- tools/adapter_sweep.py: the data path ------------------------------------------------------------------------------------
def test_sweep_rows_are_shifted_and_right_padded(tmp_path):
    import pickle
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import adapter_sweep as sw
    rng = np.random.default_rng(2)
    entries, offsets = [], []
    for n in (5, 9):
        ids = rng.integers(0, 1024, (n, 8))
        lab = ids.copy()
        lab[:2] = -100
        entries.append({"input_ids": ids.tolist(), "labels": lab.tolist()})
    with open(tmp_path / "val.pkl", "wb") as f:                     # the layout data_preprocess.process_data writes
        for e in entries:
            offsets.append(f.tell())
            pickle.dump(e, f)
    np.save(tmp_path / "val_metas.npy", np.stack([np.array(offsets), np.array([5, 9]), np.array([3, 7])]))
    rows = sw.load_rows(str(tmp_path), 151643, 16000)
    assert [r[0].shape for r in rows] == [(12, 8), (16, 8)]
    for (ids, lab), e in zip(rows, entries):
        n = len(e["input_ids"])
        for c in range(8):
            assert np.array_equal(ids[c:c + n, c], np.array(e["input_ids"])[:, c])
            assert np.array_equal(lab[c:c + n, c], np.array(e["labels"])[:, c])
            assert (np.delete(lab[:, c], np.s_[c:c + n]) == -100).all()
            assert (np.delete(ids[:, c], np.s_[c:c + n]) == (151643 if c == 0 else 1024)).all()
    (ids, mask, lab), = list(sw.batches(rows, 8, 151643))
    assert ids.shape == (2, 16, 8) and mask.sum(1).tolist() == [16, 12]           # longest first, right-padded
    assert (lab[1, 12:] == -100).all() and (ids[1, 12:, 0] == 151643).all() and (ids[1, 12:, 1:] == 1024).all()
    assert [r[0].shape[0] for r in sw.load_rows(str(tmp_path), 151643, 10)] == [10, 10]
