"""num_return_sequences (sampled takes per prompt) without a GPU: argument checks of the drop-in happen before anything
touches the device, and the two C entry points are exported and bound."""
import numpy as np
import pytest
import torch

from mtts import capi, synth


def _model(**gen):
    from modeling_asteroid import AsteroidTTSInstruct, GenerationConfig
    cfg = synth.tiny()
    return AsteroidTTSInstruct.from_state_dict(cfg, {}, GenerationConfig(eos_token_id=cfg["eos_token_id"], **gen))


def _inputs():
    ids, mask = synth.synth_prompts(synth.tiny(), 1, 2, 24, 0.3, False)
    return torch.from_numpy(ids), torch.from_numpy(mask)


def test_greedy_config_refuses_several_takes():
    """HF: greedy search has one answer per prompt.  The model sits on the CPU here, so a call that got past the checks
    would end in the missing-device RuntimeError instead."""
    ids, mask = _inputs()
    with pytest.raises(ValueError, match="num_return_sequences"):
        _model().generate(ids, mask, max_new_tokens=8, num_return_sequences=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        _model(num_return_sequences=3).generate(ids, mask, max_new_tokens=8)


def test_zero_takes_refused():
    ids, mask = _inputs()
    with pytest.raises(ValueError, match="num_return_sequences"):
        _model(do_sample=True, top_k=20).generate(ids, mask, max_new_tokens=8, num_return_sequences=0)


def test_sampled_takes_pass_the_checks():
    """With sampling on the checks pass and the call goes on to the device (absent here)."""
    ids, mask = _inputs()
    with pytest.raises(RuntimeError, match="cuda"):
        _model(do_sample=True, top_k=20).generate(ids, mask, max_new_tokens=8, num_return_sequences=2)


def test_generation_config_default_is_one_take():
    from modeling_asteroid import GenerationConfig
    assert GenerationConfig().num_return_sequences == 1
    assert GenerationConfig(num_return_sequences=4).num_return_sequences == 4


def test_takes_entry_points_exported_and_bound():
    lib = capi.lib()
    for name in ("mtts_set_takes", "mtts_slot_fork"):
        assert name in capi.exported_symbols()
        assert getattr(lib, name).argtypes is not None
    assert lib.mtts_version() >= 201
    assert lib.mtts_set_takes(None, 2) == -1              # null engine: MTTS_EINVAL, no device touched
    assert lib.mtts_slot_fork(None, 0, 1, 0, 0, None) == capi.ESTATE


def test_scheduler_refuses_zero_takes():
    from mtts.scheduler import ContinuousBatcher
    cb = ContinuousBatcher.__new__(ContinuousBatcher)
    with pytest.raises(ValueError):
        cb.run([np.zeros((9, 8), dtype=np.int64)], 4, takes=0)
