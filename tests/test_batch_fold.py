"""FRI folding factor 2^K in the batched prover, the part that needs no GPU (zk_batch_set_fold, zk_batch_get_fold,
zk_dev_fri_fold_multi_batch; DESIGN.md "Folding factor"): the symbols are exported and refuse missing handles before they touch a
device.  tests/test_gpu_batch_fold.py has the rest."""
import ctypes as C

ERR_INVALID = -1


def test_null_handles_are_refused(zk):
    lib = zk.load()
    assert lib.zk_batch_set_fold(None, 2) == ERR_INVALID
    assert lib.zk_batch_get_fold(None) == 0
    assert lib.zk_dev_fri_fold_multi_batch(None, None, None, 4, 0, 2, None, None, 1, None) == ERR_INVALID
    assert b"null" in lib.zk_last_error()


def test_symbols_are_exported(zk):
    from zkstark_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("zk_batch_set_fold", "zk_batch_get_fold", "zk_dev_fri_fold_multi_batch"):
        assert name in _lib.SYMBOLS
        assert getattr(raw, name) is not None


def test_python_surface():
    import inspect
    import zkstark_amd
    sig = inspect.signature(zkstark_amd.BatchContext.__init__)
    assert sig.parameters["fold_log"].default == 1
    assert callable(zkstark_amd.BatchContext.set_fold)
