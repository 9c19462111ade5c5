"""CPU tests of the MXFP4 side of the checkpoint reader: parse_config recognises the format under its own name and inside
compressed-tensors configs, and accepts exactly what the kernels serve (block 32, every linear but lm_head in MXFP4)."""
import numpy as np
import pytest

from vllm_rs_amd import checkpoint as ck

BASE = dict(architectures=["Qwen3ForCausalLM"], hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
            num_key_value_heads=2, vocab_size=512, torch_dtype="bfloat16")
GROUP = {"group_0": {"targets": ["Linear"], "weights": {"num_bits": 4, "type": "float", "group_size": 32}}}


@pytest.mark.parametrize("q", [
    dict(quant_method="mxfp4"),
    dict(quant_method="compressed-tensors", format="mxfp4-pack-quantized", config_groups=GROUP, ignore=["lm_head"]),
    dict(quant_method="compressed-tensors", config_groups={"group_0": dict(GROUP["group_0"], format="mxfp4-pack-quantized")}),
])
def test_parse_config_accepts_mxfp4(q):
    from vllm_rs_amd import engine as E
    cfg = ck.parse_config(dict(BASE, quantization_config=q))
    assert cfg["quant_method"] == "mxfp4" and cfg["group_size"] == 32
    mc = E.model_config(dict(cfg, num_heads=4, rope_theta=1e4, rms_norm_eps=1e-5, max_position_embeddings=128))
    assert (mc.quant_method, mc.bits, mc.group_size) == (4, 4, 32)


@pytest.mark.parametrize("q,msg", [(dict(ignore=["lm_head", "model.layers.0.mlp.down_proj"]), "16 bits"), (dict(group_size=16), "group_size")])
def test_parse_config_rejects_unserved_mxfp4(q, msg):
    with pytest.raises(ValueError, match=msg):
        ck.parse_config(dict(BASE, quantization_config=dict(q, quant_method="compressed-tensors", format="mxfp4-pack-quantized")))


def test_mxfp4_bytes_reach_the_engine_as_stored():
    a = np.arange(64, dtype=np.uint8).reshape(4, 16)
    for leaf in ("weight_packed", "weight_scale", "blocks", "scales"):
        out = ck.to_engine_tensor("model.layers.0.mlp.up_proj." + leaf, a, "u8", ck.F16)
        assert out.dtype == np.uint8 and np.array_equal(out, a)
