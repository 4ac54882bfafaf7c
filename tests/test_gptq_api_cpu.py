"""What a GPTQ request can be refused for, decided before any device is touched (no GPU needed): the options that are
not built raise by name, a dataset given by its hub name is not fetched, a model without decoder blocks is named, and
the other calibration methods keep raising on an fp model."""
import pytest
import torch

from intel_extension_for_transformers_amd.transformers import AutoRoundConfig, AwqConfig, GPTQConfig, TeqConfig
from intel_extension_for_transformers_amd.transformers.llm.quantization.utils import convert_to_quantized_model


class _Blocks(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.model = torch.nn.Module()
        self.model.layers = torch.nn.ModuleList([torch.nn.Linear(32, 32)])
        self.lm_head = torch.nn.Linear(32, 2)


class _Flat(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.linear = torch.nn.Linear(32, 2)


def _cfg(cls=GPTQConfig, **kw):
    c = cls(**kw)
    c.post_init_hip()
    return c


IDS = [torch.zeros(2, 8, dtype=torch.long)]


@pytest.mark.parametrize("option", ["use_mse_search", "true_sequential", "use_double_quant", "layer_wise"])
def test_unsupported_options_raise_by_name(option):
    with pytest.raises(NotImplementedError, match=option):
        convert_to_quantized_model(_Blocks(), _cfg(calib_dataloader=IDS, **{option: True}), device="cuda")


def test_float_weight_types_raise():
    with pytest.raises(NotImplementedError, match="nf4"):
        convert_to_quantized_model(_Blocks(), _cfg(calib_dataloader=IDS, weight_dtype="nf4"), device="cuda")


def test_hub_dataset_is_not_fetched():
    with pytest.raises(NotImplementedError, match="calib_dataloader"):
        convert_to_quantized_model(_Blocks(), _cfg(), device="cuda")
    with pytest.raises(NotImplementedError, match="calib_dataloader"):
        convert_to_quantized_model(_Blocks(), _cfg(dataset="wikitext2"), device="cuda")


def test_model_without_decoder_blocks_is_named():
    with pytest.raises(NotImplementedError, match="_Flat"):
        convert_to_quantized_model(_Flat(), _cfg(calib_dataloader=IDS), device="cuda")


def test_calibration_data_is_kept_by_reference_and_not_serialised():
    c = _cfg(calib_dataloader=IDS, n_samples=3, seq_len=5, batch_size=2)
    assert c.calib_dataloader is IDS and "calib_dataloader" not in c.to_dict()
    from intel_extension_for_transformers_amd.transformers.llm.quantization.calibration import calibration_batches

    loader = [{"input_ids": torch.arange(16).reshape(2, 8)}, (torch.arange(8),), torch.arange(8)]
    got = calibration_batches(_cfg(calib_dataloader=loader, n_samples=3, seq_len=5, batch_size=2))
    assert [tuple(b.shape) for b in got] == [(2, 5), (1, 5)]
    assert got[0][1].tolist() == [8, 9, 10, 11, 12]


@pytest.mark.parametrize("cls", [AwqConfig, TeqConfig, AutoRoundConfig])
def test_other_calibration_methods_still_raise(cls):
    with pytest.raises(NotImplementedError, match="calibration is not part"):
        convert_to_quantized_model(_Blocks(), _cfg(cls), device="cuda")
