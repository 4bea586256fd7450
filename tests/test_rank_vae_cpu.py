"""What the device ranking of the VAE, DAE and decoder-only recommenders needs no device for: the C ABI declares, binds and
exports the aae_vae_* rank calls, and the four classes offer the methods Evaluation discovers by hasattr."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAE_RANK_CALLS = ("aae_vae_predict_topk", "aae_vae_predict_ranks", "aae_vae_decode_topk", "aae_vae_decode_ranks",
                  "aae_vae_rank_max_rows", "aae_vae_rank_full_max_rows")


def test_header_prototypes_and_library_agree_on_the_vae_rank_calls():
    from aaerec import _build, _hip
    _build.build()                       # no-op when up to date; hipcc cross-compiles without a GPU
    header = open(os.path.join(ROOT, "include", "aaerec_hip.h")).read()
    declared = set(re.findall(r"^int\s+(aae_\w+)\s*\(", header, flags=re.M))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in VAE_RANK_CALLS:
        assert name in declared, name
        assert name in _hip._PROTOS, name
        assert hasattr(lib, name), name
        assert _hip._PROTOS[name][0] is ctypes.c_int
    # the signatures follow the AAE calls, plus eps_dev behind cond_dev (the decode forms and the row caps: unchanged)
    for vae, aae, extra in (("aae_vae_predict_topk", "aae_predict_topk", 1), ("aae_vae_predict_ranks", "aae_predict_ranks", 1),
                            ("aae_vae_decode_topk", "aae_decode_topk", 0), ("aae_vae_decode_ranks", "aae_decode_ranks", 0),
                            ("aae_vae_rank_max_rows", "aae_rank_max_rows", 0),
                            ("aae_vae_rank_full_max_rows", "aae_rank_full_max_rows", 0)):
        va, aa = _hip._PROTOS[vae][1], _hip._PROTOS[aae][1]
        assert len(va) == len(aa) + extra, vae
        if extra:
            assert va[:3] == aa[:3] and va[3] is ctypes.c_void_p and va[4:] == aa[3:], vae
        else:
            assert va == aa, vae
    assert re.search(r"aae_vae_predict_topk\(aae_handle h, const aae_batch\* batch, const float\* cond_dev, const float\* eps_dev,", header)
    assert _hip.ABI_VERSION == 4 and _hip.load_library().aae_abi_version() == 4      # additive: the version stays


@pytest.mark.parametrize("method", ["predict_topk", "predict_ranks"])
def test_every_mirrored_recommender_offers_the_device_ranking(method):
    from aaerec.aae import AAERecommender, DecodingRecommender
    from aaerec.dae import DAERecommender
    from aaerec.vae import VAE, VAERecommender
    for cls in (VAE, VAERecommender, DAERecommender, DecodingRecommender, AAERecommender):
        assert callable(getattr(cls, method, None)), (cls.__name__, method)
    from aaerec._hip import HipAAE
    for name in ("vae_predict_topk", "vae_predict_ranks", "vae_decode_topk", "vae_decode_ranks", "vae_rank_max_rows",
                 "vae_rank_full_max_rows"):
        assert callable(getattr(HipAAE, name, None)), name


def test_custom_ops_define_the_vae_rank_calls_beside_the_existing_ones():
    import torch
    from aaerec import ops  # noqa: F401
    for name in ("step", "encode", "predict", "predict_topk", "predict_ranks", "vae_predict_topk", "vae_predict_ranks"):
        assert hasattr(torch.ops.aaerec, name), name
