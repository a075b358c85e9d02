"""The iso-surface entry points at the C boundary (include/ngp_hip.h: ngp_iso_workspace_bytes / ngp_iso_count / ngp_iso_emit) and the opt-in switch of
jnerf_amd/mesh.py, as far as they can be checked without a GPU: symbols, workspace sizes, argument errors before any launch."""
import ctypes as C
import subprocess
import pytest
from jnerf_amd import _lib

E_ARG, E_CAPACITY = -1, -4
ONE = C.c_void_p(4096)                    # a non-null, aligned address: the calls below must fail before dereferencing it


def test_symbols_are_exported_with_signatures():
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("ngp_iso_workspace_bytes", "ngp_iso_count", "ngp_iso_emit"):
        assert f" T {name}\n" in exported, name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib().ngp_abi_version() == 3


def test_workspace_bytes_grow_with_the_lattice():
    ws = _lib.lib().ngp_iso_workspace_bytes
    assert ws(2, 2, 2) > 0
    sizes = [2, 3, 16, 17, 64, 65, 200]
    for a, b in zip(sizes[:-1], sizes[1:]):
        assert ws(b, 9, 7) >= ws(a, 9, 7) > 0 and ws(9, b, 7) >= ws(9, a, 7) > 0 and ws(9, 7, b) >= ws(9, 7, a) > 0
    assert ws(200, 200, 200) >= 6 * 200 ** 3           # a mask and a count byte and a 32-bit vertex base per point
    assert ws(1, 8, 8) == 0 and ws(2048, 1024, 1024) == 0      # shapes the calls refuse


def test_argument_errors_come_before_any_launch():
    lib = _lib.lib()
    need = lib.ngp_iso_workspace_bytes(8, 8, 8)

    def count(u=ONE, shape=(8, 8, 8), ws=ONE, n_bytes=need, counts=ONE):
        return lib.ngp_iso_count(None, u, *shape, 0.0, ws, n_bytes, counts)

    assert count(u=None) == E_ARG and b"null" in lib.ngp_last_error()
    assert count(ws=None) == E_ARG and count(counts=None) == E_ARG
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8)):
        assert count(shape=shape, n_bytes=1 << 30) == E_ARG and b"at least 2" in lib.ngp_last_error(), shape
    assert count(n_bytes=need - 1) == E_CAPACITY and b"workspace" in lib.ngp_last_error()
    for shape in ((2048, 1024, 1024), (1 << 16, 1 << 16, 2), (1 << 31, 2, 2), (4096, 4096, 128)):          # X*Y*Z >= 2^31, the last one exactly 2^31
        assert count(shape=shape, n_bytes=1 << 62) == E_CAPACITY and b"2^31" in lib.ngp_last_error(), shape

    def emit(u=ONE, shape=(8, 8, 8), ws=ONE, n_bytes=need, nv=10, nt=10, v=ONE, t=ONE):
        return lib.ngp_iso_emit(None, u, *shape, 0.0, ws, n_bytes, nv, nt, v, t)

    assert emit(v=None, t=None) == E_ARG and b"null" in lib.ngp_last_error()
    assert emit(v=None) == E_ARG and emit(t=None) == E_ARG and emit(u=None) == E_ARG and emit(ws=None) == E_ARG
    assert emit(shape=(8, 1, 8)) == E_ARG
    assert emit(n_bytes=need - 1) == E_CAPACITY
    assert emit(nv=1 << 31) == E_CAPACITY and emit(nt=1 << 31) == E_CAPACITY and b"int32" in lib.ngp_last_error()


def test_device_iso_with_smoothing_is_refused_before_any_work():
    from jnerf_amd.mesh import extract_mesh

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"extract_mesh touched runner.{name} before refusing the combination")

    with pytest.raises(ValueError, match="iso='device' with smooth=True"):
        extract_mesh(Untouchable(), resolution=8, iso="device", smooth=True)
    with pytest.raises(ValueError, match="iso must be"):
        extract_mesh(Untouchable(), resolution=8, iso="gpu")
