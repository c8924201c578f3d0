"""Host side of the keyframe feature bank's C entry points (include/idh_bank.h): the argument checks run before any launch, so they
are exercised here without a GPU - with pointers that are never followed - and the ctypes mirror is compared with the library's struct."""
import ctypes

from implicit_depth_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
P = 4096  # stands for a 16-byte-aligned device pointer; every call below is refused before it would be read


def _desc(**over):
    d = _lib.Bank()
    d.feats, d.mats, d.N, d.H, d.W, d.C = P, P, 3, 5, 7, 16
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _gather(d, slots, B=1, K=2, src=P, mats=(P, P, P), cur=(P, P)):
    arr = None if slots is None else (ctypes.c_int32 * max(len(slots), 1))(*slots)
    return _lib.lib().idh_bank_gather_fwd(None if d is None else ctypes.byref(d), arr, cur[0], cur[1], src, *mats, B, K, None)


def _commit(d, slot, feat=P, mats=(P, P, P)):
    return _lib.lib().idh_bank_commit_fwd(None if d is None else ctypes.byref(d), slot, feat, *mats, None)


def test_struct_mirror_and_symbols():
    L = _lib.lib()
    assert L.idh_sizeof_bank() == ctypes.sizeof(_lib.Bank) == 40
    assert {"idh_bank_commit_fwd", "idh_bank_gather_fwd", "idh_sizeof_bank"} <= set(_lib.declared_symbols())


def test_gather_refuses_bad_arguments():
    assert _gather(_desc(), [0, 3]) == EINVAL and _gather(_desc(), [-1, 0]) == EINVAL and _gather(_desc(), [0, 64]) == EINVAL
    for c in (0, 4, 8, 24, 48, 64):
        assert _gather(_desc(C=c), [0, 1]) == EINVAL
    assert _gather(None, [0, 1]) == EINVAL and _gather(_desc(), None) == EINVAL
    assert _gather(_desc(feats=None), [0, 1]) == EINVAL and _gather(_desc(mats=None), [0, 1]) == EINVAL
    assert _gather(_desc(feats=P + 4), [0, 1]) == EINVAL and _gather(_desc(), [0, 1], src=P + 8) == EINVAL and _gather(_desc(), [0, 1], src=None) == EINVAL
    for i in range(3):
        assert _gather(_desc(), [0, 1], mats=tuple(None if j == i else P for j in range(3))) == EINVAL
    assert _gather(_desc(), [0, 1], cur=(None, P)) == EINVAL and _gather(_desc(), [0, 1], cur=(P, None)) == EINVAL
    assert _gather(_desc(N=0), [0, 0]) == EINVAL and _gather(_desc(N=65), [0, 0]) == EINVAL
    assert _gather(_desc(H=0), [0, 0]) == EINVAL and _gather(_desc(W=-1), [0, 0]) == EINVAL
    assert _gather(_desc(), [0, 1], B=-1) == EINVAL and _gather(_desc(), [0, 1], K=-1) == EINVAL
    short = _desc()
    short.struct_size -= 8
    assert _gather(short, [0, 1]) == EINVAL
    assert _gather(_desc(), [0] * 1025, B=205, K=5) == EUNSUPPORTED  # more views than one launch's slot list holds
    assert _gather(_desc(H=1 << 14, W=1 << 14, C=16), [0, 1]) == EUNSUPPORTED
    assert _gather(_desc(), [], B=0, K=7) == 0 and _gather(_desc(), [], B=3, K=0) == 0  # nothing to do, nothing launched


def test_commit_refuses_bad_arguments():
    assert _commit(_desc(), -1) == EINVAL and _commit(_desc(), 3) == EINVAL and _commit(None, 0) == EINVAL
    assert _commit(_desc(C=8), 0) == EINVAL and _commit(_desc(), 0, feat=None) == EINVAL and _commit(_desc(), 0, feat=P + 4) == EINVAL
    for i in range(3):
        assert _commit(_desc(), 0, mats=tuple(None if j == i else P for j in range(3))) == EINVAL
    assert _commit(_desc(H=1 << 14, W=1 << 14, C=32), 0) == EUNSUPPORTED
