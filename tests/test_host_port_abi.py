"""The host-port interface without a GPU (include/gpu_actor_host.h): the
header's prototypes, pony/gpu_actor/host_port.pony's `use @` declarations and
tests/c_abi/host_port_calls.c's restatement of them agree in name, arity and
kind of every argument; the library exports them with default visibility and
each returns GPU_ACTOR_ESTATE before init; the C program compiles under
-Wall -Wextra -Werror, links -lgpuactor and passes its before-init calls;
engine.HOST_EXPORTS lists the header's names; and the emitter program the GPU
tests run reaches quiescence in the oracle with the totals its definition
gives."""
import ctypes
import os
import re
import subprocess

import numpy as np

from ponyc_amd import engine
from ponyc_amd.engine import HT_FANIN_ANALYZER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpu_actor_host.h")
PONY = os.path.join(ROOT, "pony", "gpu_actor", "host_port.pony")
CSRC = os.path.join(ROOT, "tests", "c_abi", "host_port_calls.c")
LIBDIR = os.path.dirname(engine.LIB_PATH)
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
ESTATE = -6


def _split_args(s: str) -> list:
    """top-level comma split (function-pointer and lambda types nest)"""
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return [a for a in out if a != "void"]


def _balanced(text: str, start: int) -> str:
    """text[start] is '(': the contents up to its matching ')'"""
    depth = 0
    for i in range(start, len(text)):
        if text[i] == "(":
            depth += 1
        elif text[i] == ")":
            depth -= 1
            if depth == 0:
                return text[start + 1:i]
    raise AssertionError("unbalanced")


def _c_kind(arg: str, fn_typedefs=()) -> str:
    if "(*" in arg or any(re.match(rf"{t}\b", arg) for t in fn_typedefs):
        return "fnptr"
    if "*" in arg:
        return "ptr"
    base = arg.split()[0]
    return {"uint64_t": "u64", "uint32_t": "u32", "int32_t": "i32", "int": "i32"}[base]


def _pony_kind(arg: str) -> str:
    ty = arg.split(":", 1)[1].strip()
    if ty.startswith("@{"):
        return "fnptr"
    if ty.startswith("Pointer["):
        return "ptr"
    return {"U64": "u64", "U32": "u32", "I32": "i32"}.get(ty.split()[0], "ptr")   # a tag/struct: a pointer


def header_sigs() -> dict:
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fn_typedefs = re.findall(r"typedef\s+\w+\s*\(\*(\w+)\)", text)
    out = {}
    for m in re.finditer(r"GPU_ACTOR_API\s+(\w+)\s+(\w+)\s*\(", text):
        args = _split_args(_balanced(text, m.end() - 1))
        out[m.group(2)] = (_c_kind(m.group(1) + " r"), [_c_kind(a, fn_typedefs) for a in args])
    return out


def pony_sigs() -> dict:
    text = open(PONY).read()
    out = {}
    for m in re.finditer(r"^use @(\w+)\[(\w+)\]\(", text, flags=re.M):
        args = _split_args(_balanced(text, m.end() - 1))
        out[m.group(1)] = (_pony_kind("r: " + m.group(2)), [_pony_kind(a) for a in args])
    return out


def c_sigs() -> dict:
    text = re.sub(r"/\*.*?\*/", "", open(CSRC).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^(int32_t|uint32_t|uint64_t)\s+(gpu_actor_\w+)\s*\(", text, flags=re.M):
        args = _split_args(_balanced(text, m.end() - 1))
        out[m.group(2)] = (_c_kind(m.group(1) + " r"), [_c_kind(a) for a in args])
    return out


def test_header_pony_and_c_agree():
    hdr, pony, c = header_sigs(), pony_sigs(), c_sigs()
    assert len(hdr) >= 4
    assert sorted(hdr) == sorted(pony) == sorted(c)
    for name, sig in hdr.items():
        assert pony[name] == sig, (name, pony[name], sig)
        assert c[name] == sig, (name, c[name], sig)


def test_python_exports_match_header():
    assert sorted(engine.HOST_EXPORTS) == sorted(header_sigs())
    assert not set(engine.HOST_EXPORTS) & set(engine.EXPORTS)
    m = re.search(r"#define\s+GPU_ACTOR_HT_HOST_PORT\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == engine.HT_HOST_PORT and engine.HT_HOST_PORT != 13
    assert engine.HOST_MSG_DTYPE.itemsize == 32
    assert [engine.HOST_MSG_DTYPE.fields[k][1] for k in ("step", "from", "seq", "to", "behaviour", "arg")] == \
        [0, 8, 12, 16, 20, 24]


def test_library_exports_symbols():
    r = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    defined = {l.split()[-1] for l in r.stdout.splitlines() if " T " in l}
    for name in engine.HOST_EXPORTS:
        assert name in defined, name


def test_estate_before_init():
    lib = engine.load_library()
    n = ctypes.c_uint64(5)
    buf = np.zeros(2, dtype=engine.HOST_MSG_DTYPE)
    assert lib.gpu_actor_host_reserve(1024) == ESTATE
    assert lib.gpu_actor_recv(buf.ctypes.data_as(ctypes.c_void_p), 2, ctypes.byref(n)) == ESTATE
    assert lib.gpu_actor_recv_pending(ctypes.byref(n)) == ESTATE
    assert lib.gpu_actor_host_notify(engine.HOST_FN(), None) == ESTATE


def test_c_program_links_and_calls_before_init(tmp_path):
    engine.load_library()
    exe = str(tmp_path / "host_port_calls")
    cmd = ["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", CSRC, "-o", exe,
           f"-L{LIBDIR}", "-lgpuactor", f"-Wl,-rpath,{LIBDIR}", f"-Wl,-rpath-link,{ROCM_LIB}",
           f"-Wl,-rpath,{ROCM_LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu: ok" in r.stdout


def test_emitter_program_in_the_oracle():
    """The test program itself, pinned on the CPU: stand-in A (Analyzers in
    the ports' place) reaches quiescence with the totals the definition gives."""
    import host_port_checks as H
    ref = H.stand_in(H.SMALL, "A")
    n, bursts, w = H.SMALL["n"], H.SMALL["bursts"], ref["w"]
    m = np.arange(n) % 4
    pushes = int(m.sum()) * bursts
    c = ref["counts"]
    assert c["pending"] == 0 and c["dropped"] == 0
    # every emitter handles `bursts` BURSTs (the first from the host) and
    # re-sends bursts - 1 of them; each PUSH is sent and delivered at once
    assert c["sent"] == pushes + n * (bursts - 1)
    assert c["delivered"] == pushes + n * bursts
    assert c["delivered_by_type"][w["emit_type"]] == n * bursts
    assert sum(c["delivered_by_type"][t] for t in w["port_types"]) == pushes
    assert ref["steps"] == bursts
    emit = ref["emit"]
    np.testing.assert_array_equal(emit[1], (m * bursts).astype(np.uint64))     # c
    np.testing.assert_array_equal(emit[2], np.full(n, bursts, dtype=np.uint64))
    # port (index + c) % P takes the message with argument index << 32 | c
    cnt = np.zeros(w["n_ports"], dtype=np.int64)
    xor = np.zeros(w["n_ports"], dtype=np.uint64)
    for i in range(n):
        for c_ in range(1, int(m[i]) * bursts + 1):
            p = (i + c_) % w["n_ports"]
            cnt[p] += 1
            xor[p] ^= np.uint64((i << 32) | c_)
    got = np.concatenate(ref["ports"], axis=1)
    np.testing.assert_array_equal(got[0], cnt.astype(np.uint64))
    np.testing.assert_array_equal(got[1], xor)
    # and stand-in B sees the same messages
    b = H.stand_in(H.SMALL, "B")
    np.testing.assert_array_equal(np.concatenate(b["ports"], axis=1)[1], cnt.astype(np.uint64))
