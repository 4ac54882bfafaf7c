"""The prompt form of the routed expert block through the module: a random-init Mixtral (the geometry and helpers of
tests/test_gpu_moe_model.py) whose experts take `form="prompt"` for the 7-token prompt, logits against the float64 twin
under that file's model-level bound; and the module's dispatch at its default attributes.
"""
import pytest
import torch

from tests import test_gpu_moe_model as M
from tests.test_gpu_moe_model import cases  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu


def test_mixtral_logits_through_the_prompt_form_match_the_twin(cases):  # noqa: F811
    _, q, ref = cases("mixtral")
    experts = M._experts_of(q)
    for m in experts.values():
        m.prompt_min_tokens = 1
    try:
        M._within(M._logits(q), ref, "mixtral prompt form")
    finally:
        for m in experts.values():
            del m.prompt_min_tokens


def test_a_300_token_call_takes_the_prompt_form(cases):  # noqa: F811
    from intel_extension_for_transformers_amd import qbits

    _, q, _ = cases("mixtral")
    mod = next(iter(M._experts_of(q).values()))
    assert mod.prompt_min_tokens <= 300
    g = torch.Generator().manual_seed(9)
    x = torch.randn(300, mod.hidden_dim, generator=g).cuda()
    idx = torch.randint(0, mod.num_experts, (300, 2), generator=g).cuda()
    w = torch.rand(300, 2, generator=g).cuda()
    direct = qbits.moe_forward(x, idx, w, mod.gate_up_blobs, mod.down_blobs, form="prompt")
    assert torch.equal(mod(x, idx, w).view(torch.int32), direct.view(torch.int32))
