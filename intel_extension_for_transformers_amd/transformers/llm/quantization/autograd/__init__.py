from .functions import (MatMulKBit, MoEExpertsKBit, matmul_kbit, moe_experts_ref_impl, qbits_acquire_type,  # noqa: F401
                        qbits_debug_enabled, qbits_woq_linear_backward_ref_impl, qbits_woq_linear_ref_impl)
