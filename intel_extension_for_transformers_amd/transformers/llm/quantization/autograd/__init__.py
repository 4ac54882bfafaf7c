from .functions import (MatMulKBit, matmul_kbit, qbits_acquire_type, qbits_woq_linear_backward_ref_impl,  # noqa: F401
                        qbits_woq_linear_ref_impl)
