"""CPU tests of the FP8 (E4M3 block-scaled) side of the checkpoint reader: the F8_E4M3 safetensors dtype comes back as bytes, f32
block scales stay f32, and parse_config accepts exactly the configuration the kernels serve."""
import json
import struct

import numpy as np
import pytest

from vllm_rs_amd import checkpoint as ck

BASE = dict(architectures=["Qwen3ForCausalLM"], hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
            num_key_value_heads=2, vocab_size=512, torch_dtype="bfloat16")


def test_f8_e4m3_tensor_round_trip(tmp_path):
    r = np.random.default_rng(0)
    w, s = r.integers(0, 256, size=(32, 256), dtype=np.uint8), r.random((1, 2)).astype(np.float32)
    header = {"l.q_proj.weight": {"dtype": "F8_E4M3", "shape": [32, 256], "data_offsets": [0, w.nbytes]},
              "l.q_proj.weight_scale_inv": {"dtype": "F32", "shape": [1, 2], "data_offsets": [w.nbytes, w.nbytes + s.nbytes]}}
    h = json.dumps(header).encode()
    p = tmp_path / "m.safetensors"
    p.write_bytes(struct.pack("<Q", len(h)) + h + w.tobytes() + s.tobytes())
    got = ck.read_safetensors(str(p))
    a, kind = got["l.q_proj.weight"]
    assert a.dtype == np.uint8 and np.array_equal(a, w)
    assert np.array_equal(ck.to_engine_tensor("l.q_proj.weight", a, kind, ck.BF16), w)
    sa, skind = got["l.q_proj.weight_scale_inv"]
    out = ck.to_engine_tensor("l.q_proj.weight_scale_inv", sa, skind, ck.BF16)
    assert out.dtype == np.float32 and np.array_equal(out, s)


@pytest.mark.parametrize("q", [dict(quant_method="fp8", weight_block_size=[128, 128], activation_scheme="dynamic"), dict(quant_method="fp8")])
def test_parse_config_accepts_fp8(q):
    cfg = ck.parse_config(dict(BASE, quantization_config=q))
    assert cfg["quant_method"] == "fp8" and cfg["group_size"] == 128


@pytest.mark.parametrize("q,msg", [(dict(weight_block_size=[64, 64]), "weight_block_size"), (dict(activation_scheme="static"), "static"),
                                   (dict(modules_to_not_convert=["model.layers.0.mlp.down_proj"]), "16 bits")])
def test_parse_config_rejects_unserved_fp8(q, msg):
    with pytest.raises(ValueError, match=msg):
        ck.parse_config(dict(BASE, quantization_config=dict(q, quant_method="fp8")))


def test_engine_config_maps_fp8():
    from vllm_rs_amd import engine as E
    cfg = ck.parse_config(dict(BASE, quantization_config=dict(quant_method="fp8")))
    mc = E.model_config(dict(cfg, num_heads=4, rope_theta=1e4, rms_norm_eps=1e-5, max_position_embeddings=128))
    assert (mc.quant_method, mc.bits, mc.group_size) == (3, 8, 128)
