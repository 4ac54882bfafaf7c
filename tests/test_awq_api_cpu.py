"""What an AWQ request can be refused for, decided before any device is touched (no GPU needed): the options that are
not built raise by name, auto_scale names the layout it cannot fold into, auto_clip names the group size it cannot
take, a dataset given by its hub name is not fetched; the calibration data is kept by reference and never serialised."""
import pytest
import torch

from intel_extension_for_transformers_amd.transformers import AwqConfig
from intel_extension_for_transformers_amd.transformers.llm.quantization.utils import convert_to_quantized_model

IDS = [torch.zeros(2, 8, dtype=torch.long)]


class _Cfg:
    def __init__(self, model_type):
        self.model_type = model_type


class _Blocks(torch.nn.Module):
    def __init__(self, model_type="llama"):
        super().__init__()
        self.config = _Cfg(model_type)
        self.model = torch.nn.Module()
        self.model.layers = torch.nn.ModuleList([torch.nn.Linear(32, 32)])
        self.lm_head = torch.nn.Linear(32, 2)


class _Flat(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.linear = torch.nn.Linear(32, 2)


def _cfg(**kw):
    kw.setdefault("bits", 4)
    c = AwqConfig(**kw)
    c.post_init_hip()
    return c


@pytest.mark.parametrize("option", ["use_double_quant", "layer_wise"])
def test_unsupported_options_raise_by_name(option):
    with pytest.raises(NotImplementedError, match=option):
        convert_to_quantized_model(_Blocks(), _cfg(calib_dataloader=IDS, **{option: True}), device="cuda")


def test_float_weight_types_raise():
    with pytest.raises(NotImplementedError, match="nf4"):
        convert_to_quantized_model(_Blocks(), _cfg(calib_dataloader=IDS, weight_dtype="nf4", zero_point=False),
                                   device="cuda")


def test_auto_scale_names_the_layout_it_cannot_fold_into():
    with pytest.raises(NotImplementedError, match="auto_scale.*gpt2"):
        convert_to_quantized_model(_Blocks("gpt2"), _cfg(calib_dataloader=IDS), device="cuda")
    from transformers import GPT2Config, GPT2LMHeadModel

    gpt2 = GPT2LMHeadModel(GPT2Config(n_embd=32, n_layer=1, n_head=2, vocab_size=64, n_positions=16))
    with pytest.raises(NotImplementedError, match="auto_scale.*gpt2"):
        convert_to_quantized_model(gpt2, _cfg(calib_dataloader=IDS), device="cuda")


def test_auto_clip_names_the_group_size_it_cannot_take():
    with pytest.raises(NotImplementedError, match="auto_clip.*group_size=-1"):
        convert_to_quantized_model(_Blocks(), _cfg(calib_dataloader=IDS, group_size=-1), device="cuda")


def test_hub_dataset_is_not_fetched():
    for cfg in (_cfg(), _cfg(dataset="wikitext2"), AwqConfig()):
        cfg.post_init_hip()
        with pytest.raises(NotImplementedError, match="calibration is not part.*calib_dataloader"):
            convert_to_quantized_model(_Blocks(), cfg, device="cuda")


def test_model_without_decoder_blocks_is_named():
    with pytest.raises(NotImplementedError, match="_Flat"):
        convert_to_quantized_model(_Flat(), _cfg(calib_dataloader=IDS), device="cuda")


def test_a_valid_request_passes_validation_and_only_then_asks_for_the_device():
    # everything that can be refused has been checked when the device is looked at: 'cpu' is refused last
    with pytest.raises(RuntimeError, match="no CPU path"):
        convert_to_quantized_model(_Blocks(), _cfg(calib_dataloader=IDS), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        convert_to_quantized_model(_Blocks("gpt2"), _cfg(calib_dataloader=IDS, auto_scale=False), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        convert_to_quantized_model(_Blocks(), _cfg(calib_dataloader=IDS, auto_clip=False, group_size=-1), device="cpu")


def test_calibration_data_is_kept_by_reference_and_not_serialised():
    c = _cfg(calib_dataloader=IDS, n_samples=3, seq_len=5)
    assert c.calib_dataloader is IDS and "calib_dataloader" not in c.to_dict()
    assert "calib_dataloader" not in c.to_json_string(use_diff=False)
    assert AwqConfig().calib_dataloader is None and AwqConfig.from_dict(c.to_dict()).calib_dataloader is None
    assert c.sym is False and _cfg(zero_point=False).scheme == "sym"
    from intel_extension_for_transformers_amd.transformers.llm.quantization.calibration import calibration_batches

    got = calibration_batches(_cfg(calib_dataloader=[torch.arange(16).reshape(2, 8)], n_samples=3, seq_len=5))
    assert [tuple(b.shape) for b in got] == [(1, 5), (1, 5)]  # AwqConfig has no batch_size: one row a batch
