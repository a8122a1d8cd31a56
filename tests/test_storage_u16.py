"""16-bit fixed-point storage of the methylation shard (VAMPOMI_STORE_U16), the
parts that need no device: the new entry points exist beside an unchanged ABI,
the memory plan shrinks by exactly the shard's saving (so the project's largest
configuration fits one card), VAMPOMI_STORAGE=u16 is a legal default, and
main_meth.exe parses and echoes --meth-storage u16 / --meth-dtype u16 before any
device call."""
import ctypes as C
import subprocess

import pytest

import vampomi_amd as va
from vampomi_amd import _lib

CUS = 256
SHAPES = [(10_000, 50_000, 1, 0), (100_000, 500_000, 8, 3), (1001, 517, 3, 2)]  # tests/test_storage_f32.py


def cli(*args):
    return subprocess.run([va.CLI_PATH, *args], capture_output=True, text=True, timeout=120)


def test_symbols_exist_and_abi_version_is_unchanged():
    lib = va.load()
    for name in ("vampomi_load_meth_file_u16", "vampomi_load_meth_host_u16", "vampomi_get_quant_stats"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.vampomi_abi_version() == 3
    assert va.STORE_U16 == 16
    assert (va.STORE_F64, va.STORE_F32) == (0, 1)  # existing values unchanged
    assert _lib.STATUS[9] == "ERR_RANGE" and _lib.STATUS[8] == "ERR_MODEL"
    assert hasattr(va.Data, "quant_stats")


def _plan(N, Mt, nranks, rank, probit, storage):
    b = C.c_int64()
    st = va.load().vampomi_dev_mem_plan_storage(N, Mt, nranks, rank, CUS, probit, 0, storage, C.byref(b))
    return st, b.value


@pytest.mark.parametrize("N,Mt,nranks,rank", SHAPES)
@pytest.mark.parametrize("probit", [0, 1])
def test_mem_plan_is_the_f64_plan_less_six_bytes_per_element(N, Mt, nranks, rank, probit):
    st1, f64 = _plan(N, Mt, nranks, rank, probit, va.STORE_F64)
    st2, u16 = _plan(N, Mt, nranks, rank, probit, va.STORE_U16)
    assert (st1, st2) == (0, 0)
    M, _, _ = va.divide_work(Mt, nranks, rank)
    ld = (N + 15) // 16 * 16
    assert f64 - u16 == M * ld * 6


def test_the_largest_configuration_fits_one_card_as_u16():
    """configs[2] (N = 100 000, Mt = 500 000) on one rank: 100 GB of X as u16,
    under the 288 GB of one MI355X; as floats X alone is 200 GB."""
    st1, u16 = _plan(100_000, 500_000, 1, 0, 0, va.STORE_U16)
    st2, f32 = _plan(100_000, 500_000, 1, 0, 0, va.STORE_F32)
    assert (st1, st2) == (0, 0)
    assert 100e9 < u16 < 288e9
    assert f32 > 200e9


def test_set_storage_rejects_a_null_context():
    assert va.load().vampomi_set_storage(None, va.STORE_U16) == 1


def test_u16_in_the_environment_does_not_fail_open_for_that_reason(monkeypatch):
    """VAMPOMI_STORAGE is checked before any device call: "f16" stops
    vampomi_open there with a message that names the variable; "u16" gets past
    that check (the open then succeeds, or fails for want of a device)."""
    lib = va.load()
    d = _lib.ShardDesc(N=10, Mt=10, rank=0, nranks=1, device=-1, comm_id=None, alpha_scale=1.0)
    monkeypatch.setenv("VAMPOMI_STORAGE", "f16")
    h = C.c_void_p()
    assert lib.vampomi_open(C.byref(d), C.byref(h)) == 1
    msg = lib.vampomi_last_error()
    assert b"VAMPOMI_STORAGE" in msg and b"u16" in msg  # the legal values are named
    monkeypatch.setenv("VAMPOMI_STORAGE", "u16")
    h = C.c_void_p()
    st = lib.vampomi_open(C.byref(d), C.byref(h))
    if st == 0:
        s = C.c_int(-1)
        assert lib.vampomi_get_storage(h, C.byref(s)) == 0 and s.value == va.STORE_U16
        lib.vampomi_close(h)
    else:
        assert b"VAMPOMI_STORAGE" not in lib.vampomi_last_error()


def test_data_accepts_the_name_before_any_device_call(monkeypatch):
    """Data(storage=...) checks the name first: "u16" passes that check (what
    follows needs a device), "f16" still raises ValueError."""
    with pytest.raises(ValueError):
        va.Data(10, 10, storage="f16")
    assert va._STORAGE["u16"] == va.STORE_U16


@pytest.mark.parametrize("flag", ["--meth-storage", "--meth-dtype"])
def test_cli_bad_value_names_the_three_legal_values(flag):
    r = cli("--meth-file", "m.bin", "--N", "10", "--Mt", "20", flag, "f16")
    assert r.returncode == 1
    assert "FATAL" in r.stdout and flag in r.stdout and "(f16 was passed)" in r.stdout
    assert "f64, f32 or u16" in r.stdout


@pytest.mark.parametrize("storage,dtype", [("u16", "u16"), ("u16", "f64"), ("f64", "u16"), ("f32", "u16")])
def test_cli_u16_values_are_echoed(storage, dtype):
    # (an unsupported run mode stops the program after the echo, before the device)
    r = cli("--meth-file", "m.bin", "--N", "10", "--Mt", "20", "--meth-storage", storage, "--meth-dtype", dtype,
            "--run-mode", "predict")
    assert "ardyh command line options:" in r.stdout
    assert f"--meth-storage {storage}\n" in r.stdout and f"--meth-dtype {dtype}\n" in r.stdout
    assert r.returncode == 1 and 'run mode "predict"' in r.stdout
