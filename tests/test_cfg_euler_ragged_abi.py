"""CPU: error behaviour of omni_cfg_euler_step_ragged (include/omni_cdna4.h), in the manner of tests/test_abi_error_behaviour.py:
one argument of an otherwise valid call made invalid, the documented status back BEFORE anything is launched — the pointers are
made-up addresses that are never dereferenced.  Order: null / size errors (BAD_ARG), shape limits (UNSUPPORTED), alignment
(ALIGN).  The Python wrapper refuses a library without the capability bit by name."""
import pytest

OK, BAD_ARG, UNSUPPORTED, LAUNCH, ALIGN = 0, -1, -2, -3, -4
P = 0x7F0000010000          # a "device pointer": 16-byte aligned, never dereferenced
NAME = "omni_cfg_euler_step_ragged"


def test_ragged_step_update_rejects_bad_arguments():
    from vllm_omni_amd import _native as N

    fn = getattr(N.lib(), NAME)
    # (pred, n_pred_rows, latents, n_lat_rows, lat_in, n_in_rows, reqs, R, total_rows, C, dt, n_dt, normalize, stream)
    base = [P, 1138, P, 408, P, 1138, P, 3, 408, 64, P, 3, 1, None]
    cases = [(0, None, BAD_ARG), (2, None, BAD_ARG), (4, None, BAD_ARG), (6, None, BAD_ARG), (10, None, BAD_ARG),   # pointers
             (1, 0, BAD_ARG), (3, 0, BAD_ARG), (5, -4, BAD_ARG), (7, 0, BAD_ARG), (8, 0, BAD_ARG), (11, 0, BAD_ARG),   # sizes
             (8, 409, BAD_ARG),                            # more rows to update than `latents` has
             (9, 32, UNSUPPORTED), (9, 128, UNSUPPORTED), (7, 65, UNSUPPORTED),                                      # C, R
             (0, P + 8, ALIGN), (2, P + 2, ALIGN), (4, P + 8, ALIGN), (6, P + 2, ALIGN), (10, P + 1, ALIGN)]
    for idx, val, want in cases:
        args = list(base)
        args[idx] = val
        got = fn(*args)
        assert got == want, f"{NAME}: argument {idx} = {val!r}: status {got}, expected {want}"
    # BAD_ARG before UNSUPPORTED before ALIGN
    assert fn(None, 1138, P + 2, 408, P, 1138, P, 65, 408, 32, P, 3, 1, None) == BAD_ARG
    assert fn(P + 2, 1138, P, 408, P, 1138, P, 65, 408, 64, P, 3, 1, None) == UNSUPPORTED


def test_wrapper_names_the_missing_capability(monkeypatch):
    import torch

    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    monkeypatch.setattr(N, "features", lambda: N.FEATURE_ATTN_F16 | N.FEATURE_TEACACHE_RAGGED)
    z = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(N.OmniNativeError, match="OMNI_FEATURE_CFG_EULER_RAGGED"):
        ops.cfg_euler_step_ragged_(z, z, z, torch.zeros(1, 8, dtype=torch.int32), 1, 4, torch.zeros(1))
