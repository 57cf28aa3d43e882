"""No-GPU checks of the sharded set_topology (include/wtp.h: wtp_block_knn, wtp_block_radius_*): the library exports
the three calls, the ctypes layer binds them, and the host mirror rejects bad arguments before any GPU call."""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("wtp_block_knn", "wtp_block_radius_offsets", "wtp_block_radius_fill")


def test_library_exports_and_binds_the_sharded_topology(wtp):
    lib = ctypes.CDLL(wtp.SO_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), f"libwtp.so lacks {s}"
    from whatsthepoint_jl_amd import _lib

    for s in SYMBOLS:
        assert s in _lib.SIGNATURES
    bound = _lib.load()
    for s in SYMBOLS:
        assert getattr(bound, s).argtypes == _lib.SIGNATURES[s][1]
    names = [f for f, _ in _lib.BlockTopoInfo._fields_]
    assert names == ["width", "n_ghost", "n_recv_rows", "n_peers", "widened", "host_syncs", "reserved"]
    assert ctypes.sizeof(_lib.BlockTopoInfo) == 40


class _NoContext:
    """Stands in for a Context: any use of it (a GPU call) fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the argument check touched the context ({name})")


def _share(n=16):
    rng = np.random.default_rng(0)
    return rng.random((n, 3), dtype=np.float32), np.arange(n, dtype=np.int64)


@pytest.mark.parametrize("k", [0, -3])
def test_block_knn_rejects_k_below_one(wtp, k):
    from whatsthepoint_jl_amd import blockc

    x, g = _share()
    with pytest.raises(wtp.WtpArgumentError):
        blockc.block_knn(_NoContext(), 0, 1, x, g, k)


@pytest.mark.parametrize("r", [0.0, -1.0, float("nan"), float("inf")])
def test_block_radius_rejects_bad_radius(wtp, r):
    from whatsthepoint_jl_amd import blockc

    x, g = _share()
    with pytest.raises(wtp.WtpArgumentError):
        blockc.block_radius(_NoContext(), 0, 1, x, g, r)


def _bad_shares():
    x, g = _share()
    return [
        (x[:, :2].copy(), g),                 # 2-D points
        (x.reshape(-1), g),                   # flat
        (x.astype(np.float64), g),            # fp64 (fp32 only)
        (x, g[:-1]),                          # gid length
        (x, g.astype(np.int32)),              # gid dtype
        (x, g.reshape(-1, 1)),                # gid shape
    ]


@pytest.mark.parametrize("case", range(6))
def test_block_knn_and_radius_reject_bad_shapes_and_dtypes(wtp, case):
    from whatsthepoint_jl_amd import blockc

    x, g = _bad_shares()[case]
    with pytest.raises(wtp.WtpArgumentError):
        blockc.block_knn(_NoContext(), 0, 1, x, g, 4)
    with pytest.raises(wtp.WtpArgumentError):
        blockc.block_radius(_NoContext(), 0, 1, x, g, 0.1)


def test_torch_inputs_are_checked_too(wtp):
    import torch
    from whatsthepoint_jl_amd import blockc

    x, g = _share()
    with pytest.raises(wtp.WtpArgumentError):
        blockc.block_knn(_NoContext(), 0, 1, torch.from_numpy(x).double(), torch.from_numpy(g), 4)
    with pytest.raises(wtp.WtpArgumentError):
        blockc.block_radius(_NoContext(), 0, 1, torch.from_numpy(x), torch.from_numpy(g).int(), 0.1)
