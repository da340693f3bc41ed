"""autogptq_amd -- the AutoGPTQ quantized-linear hot path, MI355X (gfx950) native.

Only what the path needs: the HIP kernels + C ABI (``csrc/`` -> ``libgptq_mi355x.so``), a ctypes
loader (``_lib``), the ``QuantLinear`` backend class (``qlinear_mi355x``), the backend selector
mirror (``import_utils``), the callers either side of the path (``model_utils``, ``fused``), the
checkpoint formats that feed it (``awq``, ``marlin``), the tensor-parallel wrappers (``tensor_parallel``) and LoRA adapters on the
quantized layers (``lora``; ``adapter_bank``: banks of adapters selected per row); ``moe``: routed experts, their router (softmax top-k, and the sigmoid /
group-limited form of DeepSeek-V3 and GLM-4 MoE) and the shared expert of Qwen-MoE and DeepSeek-V3 / GLM-4 MoE blocks.
"""
from .import_utils import MI355X_KERNELS_AVAILABLE, dynamically_import_QuantLinear  # noqa: F401
from .qlinear_mi355x import QuantLinear, reserve_workspace  # noqa: F401
from .fused import fuse_gate_up, fuse_qkv, fuse_quant_linears  # noqa: F401
from .model_utils import autogptq_post_init, load_packed_layers, make_quant, pack_model  # noqa: F401
from .lora import (LoraQuantLinear, inject_lora, load_lora_adapter, lora_forward_multi, lora_state_dict,  # noqa: F401
                   mark_only_lora_trainable, refresh_lora, set_lora_fused_backward)
from .adapter_bank import (AdapterRouting, LoraBankQuantLinear, attach_routing, inject_lora_bank, load_adapter_slot,  # noqa: F401
                           lora_bank_forward_multi)
from .moe import (inject_fused_router, inject_shared_expert, moe_route, moe_route_grouped, moe_shared_forward, remove_fused_router,  # noqa: F401
                  remove_shared_expert, router_grouped_plan)

__version__ = "0.1.0"
