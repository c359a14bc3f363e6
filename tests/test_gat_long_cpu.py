"""The pair-score entry points (csrc/gat.hip) beyond 128 nodes, through the loaded library and without a GPU: the block count that sizes the
partial-sum buffer, and the refusals (a refused call never dereferences its pointers and launches nothing)."""
import ctypes

import pytest
import torch

from scl_amd import gat, lib

CAP = 1024      # nodes per graph of the tiled matrix-core forms


def test_nblocks_is_unchanged_up_to_128_nodes_and_grows_with_n_above():
    L = lib.load()
    for N in range(1, 129):
        assert L.scl_gat_score_nblocks(N) == (N * N + 255) // 256, N
    prev = 0
    for N in range(129, CAP + 1):
        nb = L.scl_gat_score_nblocks(N)
        assert prev <= nb <= (N + 7) // 8 + 1, N      # monotone; a block owns about 8 rows i
        assert nb * 8 >= N, N                         # and never more than 8: the rows a block keeps in LDS
        prev = nb
    # the partial sums of the largest graph at the training batch stay small: B * nblocks rows of Do * D + 4 * Do floats
    assert 64 * L.scl_gat_score_nblocks(CAP) * (64 * 64 + 4 * 64) * 4 < 1 << 28


def test_backward_names_its_scratch_bound_instead_of_failing_in_the_allocator():
    class Ctx:      # shapes only: the bound is checked before anything is allocated or launched
        n1, na = 1000, 1
        saved_tensors = (torch.empty(128, 1000, 64, device="meta"), torch.empty(64, 64, device="meta"), torch.empty(64, device="meta"),
                         torch.empty(3, 64, device="meta"))
    assert 128 * 1000 * 1000 * 64 * 4 > gat.MAX_DP_BYTES >= 64 * 999 * 999 * 64 * 4      # the training batch at the longest clip fits
    with pytest.raises(ValueError, match="%d GiB" % (gat.MAX_DP_BYTES >> 30)):
        gat._GatScoreFn.backward(Ctx, torch.empty(128, 1000, 1000, device="meta"))


def test_refusals_beyond_the_cap_of_the_scalar_forms_and_of_null_pointers():
    L = lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # a host address: a refused call never dereferences it
    err = lambda: L.scl_last_error()
    fwd = lambda x=p, W=p, bias=p, a=p, s=p, B=2, N=CAP + 1, D=64, Do=64, n1=None: \
        L.scl_gat_score_fwd(x, W, bias, a, s, B, N, D, Do, N if n1 is None else n1, None)
    bwd = lambda x=p, W=p, bias=p, a=p, ds=p, dP=p, part=p, dx=p, B=2, N=CAP + 1, D=64, Do=64, n1=None: \
        L.scl_gat_score_bwd(x, W, bias, a, ds, dP, part, dx, B, N, D, Do, N if n1 is None else n1, None)
    # cap + 1 names the cap, for every matrix-core form
    for D, Do in ((64, 64), (64, 32), (32, 32)):
        assert fwd(D=D, Do=Do) == -1 and b"gat_score_fwd" in err() and str(CAP).encode() in err(), err()
        assert bwd(D=D, Do=Do) == -1 and b"gat_score_bwd" in err() and str(CAP).encode() in err(), err()
    # the scalar forms keep byte-wide pair indices: 128 nodes, with their message
    for N in (129, 171, CAP):
        assert fwd(N=N, D=32, Do=17, n1=100) == -1 and b"gat_score_fwd" in err() and b"N <= 128" in err(), err()
        assert bwd(N=N, D=32, Do=17, n1=100) == -1 and b"gat_score_bwd" in err() and b"N <= 128" in err(), err()
        assert fwd(N=N, D=32, Do=64) == -1 and b"N <= 128" in err(), err()
    # null pointers and bad sizes, at a size only the tiled forms take
    for rc in (fwd(x=None, N=171), fwd(W=None, N=171), fwd(bias=None, N=171), fwd(a=None, N=171), fwd(s=None, N=171), fwd(B=0, N=171),
               fwd(N=171, n1=172), fwd(N=171, n1=-1), fwd(N=171, D=48)):
        assert rc == -1 and b"gat_score_fwd" in err(), err()
    for rc in (bwd(x=None, N=171), bwd(W=None, N=171), bwd(bias=None, N=171), bwd(a=None, N=171), bwd(ds=None, N=171), bwd(dP=None, N=171),
               bwd(part=None, N=171), bwd(dx=None, N=171), bwd(B=0, N=171), bwd(N=171, n1=172), bwd(N=171, D=48)):
        assert rc == -1 and b"gat_score_bwd" in err(), err()
    # the variable-length scoring entry keeps its 128 nodes
    assert L.scl_gat_score_fwd_var(p, p, p, p, p, p, None, 2, 129, 64, 64, None) == -1 and b"scl_gat_score_fwd_var" in err()
