"""Per-dialogue adapters, the parts that need no GPU: `mtts.adapters.delta_spec` (the definition the device kernel is
compared with bit for bit, tests/test_multi_adapter_gpu.py) against plain matrix products, and the argument errors of
load_adapter(adapter_name=...) / generate(adapter_names=...), which are raised before an engine exists."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mtts import adapters, synth  # noqa: E402

CFG = synth.tiny()


@pytest.mark.parametrize("K", [48, 144, 256, 2048])
@pytest.mark.parametrize("r", [1, 16, 33, 64])
def test_delta_spec_is_the_product_where_sums_are_exact(K, r):
    """Multiples of 1/8 in [-1, 1]: every product is a multiple of 1/64 and every partial sum stays far below 2^24 / 64, so
    each fp32 operation of any summation order is exact and the spec must equal the product as numpy computes it."""
    rng = np.random.default_rng(K + r)
    x, A, B = (rng.integers(-8, 9, sh).astype(np.float32) / 8 for sh in ((7, K), (r, K), (80, r)))
    want = ((x.astype(np.float64) @ A.T.astype(np.float64)) @ B.T.astype(np.float64)) * 0.25
    got = adapters.delta_spec(x, A, B, 0.25)
    assert got.dtype == np.float32 and got.shape == (7, 80)
    assert np.array_equal(got, want.astype(np.float32)) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert np.array_equal(got, ((x @ A.T) @ B.T) * np.float32(0.25))
    # one row alone gives that row: nothing depends on the other rows
    assert np.array_equal(adapters.delta_spec(x[3], A, B, 0.25), got[3])


@pytest.mark.parametrize("K,r", [(256, 16), (144, 33), (6144, 16)])
def test_delta_spec_agrees_with_the_unmerged_peft_forward(K, r):
    """PEFT's unmerged LoRA forward in fp32, lora_B(lora_A(x)) * scaling, as torch computes it: equal to fp32 rounding.
    Bound: each of the two sums carries at most (terms) * 2^-24 relative to the sum of the magnitudes of its terms."""
    rng = np.random.default_rng(3 * K + r)
    x = synth.round_bf16(rng.standard_normal((5, K)).astype(np.float32))
    A = (rng.standard_normal((r, K)) * 0.1).astype(np.float32)
    B = (rng.standard_normal((96, r)) * 0.1).astype(np.float32)
    s = 2.7
    got = adapters.delta_spec(x, A, B, s)
    ref = (torch.nn.functional.linear(torch.nn.functional.linear(torch.from_numpy(x), torch.from_numpy(A)), torch.from_numpy(B)) * s).numpy()
    mag = ((np.abs(x).astype(np.float64) @ np.abs(A).T.astype(np.float64)) @ np.abs(B).T.astype(np.float64)) * s
    assert np.all(np.abs(got.astype(np.float64) - ref) <= (K + r + 2) * 2.0 ** -23 * mag)
    # and against float64, each within its own bound
    ref64 = ((x.astype(np.float64) @ A.T.astype(np.float64)) @ B.T.astype(np.float64)) * s
    assert np.all(np.abs(got - ref64) <= (K + r + 2) * 2.0 ** -24 * mag)


def test_delta_spec_zero_b_is_zero():
    rng = np.random.default_rng(1)
    x, A = rng.standard_normal((3, 48)).astype(np.float32), rng.standard_normal((4, 48)).astype(np.float32)
    assert not adapters.delta_spec(x, A, np.zeros((32, 4), np.float32), 2.0).any()


def _name(layer, proj):
    return f"model.language_model.layers.{layer}.{proj}.weight"


def _pair(proj, r=8, seed=0):
    rng = np.random.default_rng(seed)
    o, i = adapters.projection_shape(CFG, proj)
    return (rng.standard_normal((r, i)).astype(np.float32), rng.standard_normal((o, r)).astype(np.float32))


def _model(dtype="bf16"):
    import modeling_asteroid as ma
    w = {name: np.zeros(shape, np.float32) for name, shape, _ in synth.weight_shapes(CFG)}
    return ma.AsteroidTTSInstruct.from_state_dict(CFG, w, dtype=dtype)


def test_named_adapter_bookkeeping_and_errors_need_no_engine():
    m = _model()
    good = {_name(0, "self_attn.q_proj"): _pair("self_attn.q_proj"), _name(1, "mlp.down_proj"): _pair("mlp.down_proj")}
    assert m.load_adapter(good, scaling=2.0, adapter_name="x") is m
    m.load_adapter(good, scaling=0.5, adapter_name="y")
    assert m.adapter_names() == ["x", "y"] and m._adapter is None and m._engine is None
    assert [m._named[n][0] for n in ("x", "y")] == [0, 1]
    m.load_adapter(good, scaling=1.0, adapter_name="x")                  # replaced in place
    assert m.adapter_names() == ["x", "y"] and m._named["x"][0] == 0 and m._named["x"][2] == 1.0
    m.delete_adapter("x")
    m.load_adapter(good, scaling=1.0, adapter_name="z")                  # takes the freed place
    assert m.adapter_names() == ["y", "z"] and m._named["z"][0] == 0
    with pytest.raises(ValueError, match="no resident adapter 'x'"):
        m.delete_adapter("x")
    # the same things are refused by name as without adapter_name
    with pytest.raises(ValueError, match="input_layernorm"):
        m.load_adapter({_name(0, "input_layernorm"): _pair("self_attn.q_proj")}, scaling=1.0, adapter_name="w")
    with pytest.raises(ValueError, match="needs scaling"):
        m.load_adapter(good, adapter_name="w")
    A, B = _pair("self_attn.k_proj")
    with pytest.raises(ValueError, match=r"k_proj.*\[256, 128\]"):
        m.load_adapter({_name(0, "self_attn.k_proj"): (A[:, :128], B)}, scaling=1.0, adapter_name="w")
    # resident adapters: rank at most 64, a name that is not the base's, bf16, 16 places
    with pytest.raises(ValueError, match="rank 65 is above 64"):
        m.load_adapter({_name(0, "self_attn.q_proj"): _pair("self_attn.q_proj", r=65)}, scaling=1.0, adapter_name="w")
    with pytest.raises(ValueError, match="__base__"):
        m.load_adapter(good, scaling=1.0, adapter_name="__base__")
    for dtype in ("fp32", "fp16"):
        with pytest.raises(ValueError, match="bf16 engine only, this model is " + dtype):
            _model(dtype).load_adapter(good, scaling=1.0, adapter_name="w")
    for i in range(14):
        m.load_adapter(good, scaling=1.0, adapter_name=f"n{i}")
    with pytest.raises(ValueError, match="16 adapters are resident"):
        m.load_adapter(good, scaling=1.0, adapter_name="one_too_many")
    assert "w" not in m.adapter_names() and len(m.adapter_names()) == 16 and m._engine is None


def test_generate_adapter_names_errors_come_before_any_engine():
    m = _model()            # on the CPU: reaching the engine would raise RuntimeError (model.to('cuda'))
    m.load_adapter({_name(0, "self_attn.q_proj"): _pair("self_attn.q_proj")}, scaling=1.0, adapter_name="x")
    ids, mask = synth.synth_prompts(CFG, 1, batch=3, prompt_len=16)
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    with pytest.raises(ValueError, match="adapter_names has 2 entries for a batch of 3"):
        m.generate(ids, mask, max_new_tokens=4, adapter_names=["x", "x"])
    with pytest.raises(ValueError, match="no resident adapter 'nope'"):
        m.generate(ids, mask, max_new_tokens=4, adapter_names=["x", "nope", None])
    m.generation_config.do_samples = [True] * 8
    with pytest.raises(ValueError, match="adapter_names has 6 entries"):      # one per prompt, not per take
        m.generate(ids, mask, max_new_tokens=4, num_return_sequences=2, adapter_names=["x"] * 6)
    m32 = _model("fp32")
    with pytest.raises(ValueError, match="bf16 engine only, this model is fp32"):
        m32.generate(ids, mask, max_new_tokens=4, adapter_names=[None, "__base__", None])
    # well-formed arguments get as far as the engine, which a CPU model does not have
    with pytest.raises(RuntimeError, match="cuda"):
        m.generate(ids, mask, max_new_tokens=4, adapter_names=["x", "__base__", None])
    assert m._engine is None


def test_process_batch_passes_adapter_names_through():
    import inspect

    import generation_utils
    assert inspect.signature(generation_utils.process_batch).parameters["adapter_names"].default is None


def test_parity_gate_leaves_out_at_most_a_tenth_of_the_merged_runs_decisions():
    """The case of tests/test_multi_adapter_gpu.py::test_unmerged_row_against_the_merged_adapter, on the CPU: the oracle's
    greedy run on merge_spec weights.  The adapter seed is chosen so that the 0.008 gate excludes at most 10 % of the free
    decisions of the 48 steps, and nobody leaves the speech range."""
    import multi_adapter_case as case
    from oracle import asteroid_oracle as ao
    ids, mask = case.prompts(case.PARITY_PROMPT[:1], case.PARITY_PROMPT[1])
    orc = ao.AsteroidOracle(case.CFG, case.merged_weights(1), "bf16")
    out = orc.generate(ids, mask, ids.shape[1] + case.PARITY_STEPS + 20, max_steps=case.PARITY_STEPS)
    margins = np.stack(orc.last_margins)[:case.PARITY_STEPS]
    assert margins.shape == (case.PARITY_STEPS, 1, 8)
    free = case.free_decisions(case.PARITY_STEPS)
    below = int((free & (margins < case.PARITY_GATE)).sum())
    print("free decisions %d, below the gate %d" % (int(free.sum()), below))
    assert below <= 0.1 * free.sum()
    lo, hi = case.CFG["speech_token_range"]
    gen0 = out[0, ids.shape[1] - 7:, 0]
    assert ((gen0 >= lo) & (gen0 < hi)).all()
