"""fp32 storage of the methylation shard, the parts that need no device: the
new entry points exist beside an unchanged ABI, the memory plan shrinks by
exactly the shard's saving, and main_meth.exe parses, checks and echoes
--meth-storage / --meth-dtype before any device call."""
import ctypes as C
import subprocess

import pytest

import vampomi_amd as va
from vampomi_amd import _lib

CUS = 256
SHAPES = [(10_000, 50_000, 1, 0), (100_000, 500_000, 8, 3), (1001, 517, 3, 2)]


def cli(*args):
    return subprocess.run([va.CLI_PATH, *args], capture_output=True, text=True, timeout=120)


def test_symbols_exist_and_abi_version_is_unchanged():
    lib = va.load()
    for name in ("vampomi_set_storage", "vampomi_get_storage", "vampomi_load_meth_host_f32",
                 "vampomi_load_meth_file_f32", "vampomi_dev_mem_plan_storage"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.vampomi_abi_version() == 3
    assert (va.STORE_F64, va.STORE_F32) == (0, 1)


def _plan(N, Mt, nranks, rank, probit, storage=None):
    b = C.c_int64()
    lib = va.load()
    if storage is None:
        st = lib.vampomi_dev_mem_plan(N, Mt, nranks, rank, CUS, probit, 0, C.byref(b))
    else:
        st = lib.vampomi_dev_mem_plan_storage(N, Mt, nranks, rank, CUS, probit, 0, storage, C.byref(b))
    return st, b.value


@pytest.mark.parametrize("N,Mt,nranks,rank", SHAPES)
@pytest.mark.parametrize("probit", [0, 1])
def test_mem_plan_by_storage(N, Mt, nranks, rank, probit):
    st0, old = _plan(N, Mt, nranks, rank, probit)
    st1, f64 = _plan(N, Mt, nranks, rank, probit, va.STORE_F64)
    st2, f32 = _plan(N, Mt, nranks, rank, probit, va.STORE_F32)
    assert (st0, st1, st2) == (0, 0, 0)
    assert f64 == old
    M, _, _ = va.divide_work(Mt, nranks, rank)
    ld = (N + 15) // 16 * 16
    assert f64 - f32 == M * ld * 4


@pytest.mark.parametrize("storage", [-1, 2, 7])
def test_mem_plan_rejects_a_bad_storage(storage):
    st, _ = _plan(1001, 517, 1, 0, 0, storage)
    assert st == 1  # VAMPOMI_ERR_ARG


def test_set_storage_rejects_a_null_context():
    lib = va.load()
    assert lib.vampomi_set_storage(None, va.STORE_F32) == 1
    s = C.c_int()
    assert lib.vampomi_get_storage(None, C.byref(s)) == 1


def test_bad_storage_in_the_environment_fails_open(monkeypatch):
    """VAMPOMI_STORAGE is read before any device call, so this needs no GPU."""
    monkeypatch.setenv("VAMPOMI_STORAGE", "f16")
    lib = va.load()
    h = C.c_void_p()
    d = _lib.ShardDesc(N=10, Mt=10, rank=0, nranks=1, device=-1, comm_id=None, alpha_scale=1.0)
    assert lib.vampomi_open(C.byref(d), C.byref(h)) == 1
    assert b"VAMPOMI_STORAGE" in lib.vampomi_last_error()


def test_data_rejects_a_bad_storage_name():
    with pytest.raises(ValueError):
        va.Data(10, 10, storage="f16")


@pytest.mark.parametrize("flag,val", [("--meth-storage", "f16"), ("--meth-dtype", "x")])
def test_cli_bad_value_is_fatal_with_the_flag_named(flag, val):
    r = cli("--meth-file", "m.bin", "--N", "10", "--Mt", "20", flag, val)
    assert r.returncode == 1
    assert "FATAL" in r.stdout and flag in r.stdout and f"({val} was passed)" in r.stdout


@pytest.mark.parametrize("storage,dtype", [("f32", "f32"), ("f64", "f32"), ("f32", "f64")])
def test_cli_valid_values_are_echoed(storage, dtype):
    # (an unsupported run mode stops the program after the echo, before the device)
    r = cli("--meth-file", "m.bin", "--N", "10", "--Mt", "20", "--meth-storage", storage, "--meth-dtype", dtype,
            "--run-mode", "predict")
    assert "ardyh command line options:" in r.stdout
    assert f"--meth-storage {storage}\n" in r.stdout and f"--meth-dtype {dtype}\n" in r.stdout
    assert r.returncode == 1 and 'run mode "predict"' in r.stdout
