"""zk_batch_set_ext / zk_batch_get_ext and the three probes of the batch over E (zk_dev_compose_ext_batch, zk_dev_fri_fold_multi_ext_batch,
zk_dev_merkle_build_coset_ext_batch) without a GPU: declared in the header with their exact signatures, exported by the built
library, named by the Rust file, their null-handle answers, the Python surface, and an ABI version that did not move (the setting is
additive and off by default)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTERS = ("zk_batch_set_ext", "zk_batch_get_ext")
PROBES = ("zk_dev_compose_ext_batch", "zk_dev_fri_fold_multi_ext_batch", "zk_dev_merkle_build_coset_ext_batch")
ERR_INVALID = -1


def _header():
    return open(os.path.join(ROOT, "include", "zkstark_amd.h")).read()


def test_declared_in_the_header():
    text = _header()
    assert re.search(r"^int zk_batch_set_ext\(zk_batch \*b, uint32_t ext_log\);$", text, re.M)
    assert re.search(r"^uint32_t zk_batch_get_ext\(const zk_batch \*b\);$", text, re.M)


def test_the_probes_are_declared_in_the_dev_section():
    text = _header()
    dev = text[text.index("int zk_dev_fri_fold_multi_batch("):]              # the zk_dev_* section, from the probe they are modelled on
    for name in PROBES:
        assert re.search(r"^int " + name + r"\(const ", dev, re.M), name


def test_exported_by_the_library(zk):
    raw = C.CDLL(os.path.join(ROOT, "zkstark_amd", "libzkstark_amd.so"))
    for name in SETTERS + PROBES:
        assert getattr(raw, name) is not None                # AttributeError: the symbol is missing
        assert hasattr(zk.load(), name)


def test_named_by_the_rust_bindings():
    text = open(os.path.join(ROOT, "bindings", "rust", "zkstark_amd_sys.rs")).read()
    for name in SETTERS + PROBES:
        assert re.search(r"\bpub fn " + name + r"\(", text), name


def test_null_handle(zk):
    lib = zk.load()
    for ext_log in (0, 1, 2):
        assert lib.zk_batch_set_ext(None, ext_log) == ERR_INVALID
    assert lib.zk_batch_get_ext(None) == 0


def test_the_probes_refuse_null_arguments(zk):
    lib = zk.load()
    assert lib.zk_dev_compose_ext_batch(None, None, None, None, None, None, None, 1, None) == ERR_INVALID
    assert lib.zk_dev_fri_fold_multi_ext_batch(None, None, None, 4, 0, 2, None, None, 1, None) == ERR_INVALID
    assert lib.zk_dev_merkle_build_coset_ext_batch(None, 4, 1, 1, None, None, 0) == ERR_INVALID


def test_python_takes_the_setting(zk):
    import inspect
    sig = inspect.signature(zk.BatchContext.__init__).parameters
    assert "ext_log" in sig and sig["ext_log"].default == 0
    assert hasattr(zk.BatchContext, "set_ext")


def test_the_wording_of_the_refusal_is_the_one_call_provers(zk):
    """zk_batch_set_ext(b, 2) answers with zk_ctx_set_ext's words; without a handle only the source can be read."""
    src = open(os.path.join(ROOT, "zkstark_amd", "csrc", "batch.hip")).read()
    one = open(os.path.join(ROOT, "zkstark_amd", "csrc", "zkstark.hip")).read()
    tail = "ext_log must be 0 or 1 (got %u; 2, the quartic extension, is reserved)"
    assert "zk_ctx_set_ext: " + tail in one and "zk_batch_set_ext: " + tail in src


def test_abi_version_is_unchanged(zk):
    assert zk.load().zk_abi_version() == 6
