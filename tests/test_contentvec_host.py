"""CPU checks of the ContentVec front-end (serenade_amd/contentvec.py) against transformers' HubertModel: frame counts
with the 10 ms stride override, the state-dict mapping (both weight-norm spellings, the folded positional weight) and the
kernel route of every contraction of a full-geometry plan.  Nothing here opens the GPU."""
import ctypes

import pytest
import torch

from serenade_amd import _lib
from serenade_amd.contentvec import ContentVec, _Plan, _nearest_index

transformers = pytest.importorskip("transformers")

SMALL = dict(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, conv_dim=[16] * 7,
             num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)


def _hubert(config, seed=0, final_proj=False):
    torch.manual_seed(seed)
    cfg = transformers.HubertConfig(**config)
    m = transformers.HubertModel(cfg).eval()
    m.feature_extractor.conv_layers[-1].conv.stride = (1,)  # preprocess.py:366-368
    sd = dict(m.state_dict())
    if final_proj:  # HubertModelWithFinalProj (preprocess.py:41-50)
        fp = torch.nn.Linear(cfg.hidden_size, cfg.classifier_proj_size)
        sd.update({"final_proj." + k: v for k, v in fp.state_dict().items()})
    return m, sd


@pytest.mark.parametrize("n", [400, 401, 404, 405, 409, 410, 555, 1599, 1600, 1601, 4001, 6397, 16000, 16001, 37913,
                               48000, 99999, 160000, 479999, 480000])
def test_frames_match_transformers_with_the_stride_override(n):
    m, _ = _hubert(dict(SMALL, num_hidden_layers=0, conv_dim=[4] * 7))
    with torch.no_grad():
        T = m(torch.zeros(1, n)).last_hidden_state.shape[1]
    assert ContentVec(device="cpu").frames(n) == T
    assert ContentVec(device="cpu").layer_frames(n)[-1] == T


def test_too_short_input_has_no_frames():
    assert ContentVec(device="cpu").frames(399) == 0


def _unpack_pos(cv):
    c = cv.config
    D, G, K = c["hidden_size"], c["num_conv_pos_embedding_groups"], c["num_conv_pos_embeddings"]
    Cg = D // G
    p = cv.w["pos_w"][..., :Cg]  # [g][tap][c in][n out]
    return p.permute(0, 3, 2, 1).reshape(D, Cg, K)


@pytest.mark.parametrize("spelling", ["parametrizations", "hub"])
def test_state_dict_mapping_and_folded_positional_weight(spelling):
    m, sd = _hubert(SMALL, seed=3, final_proj=True)
    with torch.no_grad():  # a weight norm with non-trivial g
        m.encoder.pos_conv_embed.conv.parametrizations.weight.original0.mul_(1.7)
    sd = dict(m.state_dict(), **{k: v for k, v in sd.items() if k.startswith("final_proj.")})
    pre = "encoder.pos_conv_embed.conv."
    if spelling == "hub":
        sd[pre + "weight_g"] = sd.pop(pre + "parametrizations.weight.original0")
        sd[pre + "weight_v"] = sd.pop(pre + "parametrizations.weight.original1")
    cv = ContentVec(device="cpu", **SMALL).load_state_dict(sd)
    ref = m.encoder.pos_conv_embed.conv.weight.detach()
    assert (_unpack_pos(cv) - ref).abs().max().item() <= 1e-7
    assert torch.equal(cv.w["layers"][0]["qkv_w"][: SMALL["hidden_size"]], sd["encoder.layers.0.attention.q_proj.weight"])
    assert cv.w["pos_w"].shape[-1] == 32  # columns padded to the kernel's 32-wide block


def test_unexpected_or_missing_key_raises():
    _, sd = _hubert(SMALL, seed=1)
    cv = ContentVec(device="cpu", **SMALL)
    with pytest.raises(KeyError, match="unexpected"):
        cv.load_state_dict(dict(sd, **{"encoder.extra.weight": torch.zeros(1)}))
    sd2 = dict(sd)
    del sd2["encoder.layer_norm.bias"]
    with pytest.raises(KeyError, match="missing"):
        cv.load_state_dict(sd2)
    cv.load_state_dict(dict(sd, masked_spec_embed=torch.zeros(SMALL["hidden_size"])))  # ignored


def test_unsupported_geometry_raises():
    with pytest.raises(ValueError):
        ContentVec(device="cpu", do_stable_layer_norm=True)
    with pytest.raises(ValueError):
        ContentVec(device="cpu", feat_extract_norm="layer")
    with pytest.raises(TypeError):
        ContentVec(device="cpu", not_a_setting=1)


def test_every_contraction_of_a_full_plan_routes_to_a_family_with_gelu():
    """all five srn_conv_gemm families apply SRN_POST_GELU; the route must still be a known family for every op of the
    hubert-base plan, with and without a split-K workspace"""
    _, sd = _hubert({}, seed=0)
    cv = ContentVec(device="cpu").load_state_dict(sd)
    lengths = [16000, 23700, 48000]
    plan = _Plan(cv, torch.device("cpu"), 3, 48000, lengths)
    h = _lib.lib()
    gelu_families = {_lib.FAMILY_GENERIC, _lib.FAMILY_F32, _lib.FAMILY_FAST, _lib.FAMILY_HALO, _lib.FAMILY_STRIP}
    seen = 0
    n_gelu = 0
    for op in plan.ops:
        if not hasattr(op, "p"):
            continue
        for ws in (False, True):
            p = _lib.SrnConvParams.from_buffer_copy(op.p)
            if ws:
                p.ws, p.ws_bytes = 16, 1 << 40
            out = (ctypes.c_int32 * 3)()
            assert h.srn_conv_gemm_route(ctypes.byref(p), out) == 0, h.srn_last_error()
            assert out[0] in gelu_families
        seen += 1
        n_gelu += op.p.post == _lib.POST_GELU
    assert seen > 12 * 4 and n_gelu == 6 + 12  # feature convs 1-6 and every feed-forward


@pytest.mark.parametrize("n_in,scale", [(100, 1.0), (98, 1.0), (77, 0.75), (50, 2.0), (61, 1.3333333333333333)])
def test_nearest_index_matches_torch_interpolate(n_in, scale):
    x = torch.arange(n_in, dtype=torch.float32).view(1, 1, -1)
    ref = torch.nn.functional.interpolate(x, scale_factor=scale)[0, 0].long().numpy()
    assert (_nearest_index(n_in, scale) == ref).all()
