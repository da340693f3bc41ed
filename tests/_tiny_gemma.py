"""A randomly initialised tiny Gemma (GeGLU MLP: down(gelu_tanh(gate(x)) * up(x)), three projections per block), quantised and packed the way _tiny_llama
does it for the tiny Llama -- the oracle's min/max quantizer, this backend's pack_model."""
import torch

from _tiny_llama import quantize_and_pack      # noqa: F401  (works on any model whose quantised linears live under model.layers.)


def tiny_config():
    from transformers import GemmaConfig
    return GemmaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, head_dim=64,
                       vocab_size=512, max_position_embeddings=128, attn_implementation="eager", tie_word_embeddings=False)


def fresh_model(seed):
    from transformers import GemmaForCausalLM
    torch.manual_seed(seed)
    m = GemmaForCausalLM(tiny_config())
    m.lm_head.weight.data.normal_(0, 0.3)          # spread the logits: greedy argmax is then far from ties
    return m.half().eval()
