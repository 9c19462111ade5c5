"""CPU tests of the NVFP4 side of the checkpoint reader: parse_config recognises the format under its own name, as ModelOpt and inside
compressed-tensors configs, accepts exactly what the kernels serve (group 16, every linear but lm_head in NVFP4), and the tensors
reach the engine as stored: bytes as bytes, the per-tensor scales as f32."""
import numpy as np
import pytest

from vllm_rs_amd import checkpoint as ck

BASE = dict(architectures=["Qwen3ForCausalLM"], hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
            num_key_value_heads=2, vocab_size=512, torch_dtype="bfloat16")
GROUP = {"group_0": {"targets": ["Linear"], "weights": {"num_bits": 4, "type": "float", "group_size": 16}}}
CT = dict(quant_method="compressed-tensors", format="nvfp4-pack-quantized")


@pytest.mark.parametrize("q", [
    dict(quant_method="nvfp4"),
    dict(quant_method="modelopt", quant_algo="NVFP4", exclude_modules=["lm_head"]),
    dict(quant_method="modelopt", quantization={"quant_algo": "fp4", "group_size": 16}),
    dict(CT, config_groups=GROUP, ignore=["lm_head"]),
    dict(quant_method="compressed-tensors", config_groups={"group_0": dict(GROUP["group_0"], format="nvfp4-pack-quantized")}),
    dict(quant_method="compressed-tensors", config_groups={"group_0": {"weights": dict(GROUP["group_0"]["weights"], format="nvfp4-pack-quantized")}}),
])
def test_parse_config_accepts_nvfp4(q):
    from vllm_rs_amd import engine as E
    cfg = ck.parse_config(dict(BASE, quantization_config=q))
    assert cfg["quant_method"] == "nvfp4" and cfg["group_size"] == 16
    mc = E.model_config(dict(cfg, num_heads=4, rope_theta=1e4, rms_norm_eps=1e-5, max_position_embeddings=128))
    assert (mc.quant_method, mc.bits, mc.group_size) == (5, 4, 16)


@pytest.mark.parametrize("q,msg", [(dict(CT, ignore=["lm_head", "model.layers.0.mlp.down_proj"]), "16 bits"), (dict(CT, group_size=32), "group_size"),
                                   (dict(quant_method="mlx", mode="nvfp4"), "not on this path")])
def test_parse_config_rejects_unserved_nvfp4(q, msg):
    with pytest.raises(ValueError, match=msg):
        ck.parse_config(dict(BASE, quantization_config=q))


def test_nvfp4_tensors_reach_the_engine_as_stored():
    a = np.arange(64, dtype=np.uint8).reshape(4, 16)
    for leaf, kind in (("weight_packed", "u8"), ("weight", "u8"), ("weight_scale", "f8e4m3"), ("weight_scale", "u8")):
        out = ck.to_engine_tensor("model.layers.0.mlp.up_proj." + leaf, a, kind, ck.F16)
        assert out.dtype == np.uint8 and np.array_equal(out, a)
    s = np.array([2688.0 * 448.0 / 3.1], np.float32)  # (would overflow f16 and lose bits in bf16)
    for leaf in ("weight_global_scale", "weight_scale_2", "input_scale", "input_global_scale"):
        for dt in (ck.BF16, ck.F16):
            out = ck.to_engine_tensor("model.layers.0.mlp.up_proj." + leaf, s, "f32", dt)
            assert out.dtype == np.float32 and np.array_equal(out, s)
