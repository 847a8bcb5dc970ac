"""Kernarg preload of the decode kernels, read from the kernel descriptors of the built library.

The library is compiled with ``-amdgpu-kernarg-preload-count=16`` (ops/build.py): the leading
kernel-argument dwords arrive in user SGPRs, at most 14 of them and only the pointers and scalars ahead
of the first by-value struct (docs/KERNARG_PRELOAD.md).  The decode kernels therefore list first what a
wave's first loads need.  This test reads, for EVERY instantiation of each kernel family in the
library, the descriptor's ``kernarg_preload_length`` (llvm-objdump prints the ``.kd`` symbols of the
extracted gfx950 code objects as ``.amdhsa_*`` directives) and asserts that it covers the dwords
counted below.  Descriptors only: no instruction stream is read.

Dwords a family's first loads need (an 8-byte argument is two dwords and starts on an even dword):

* ``gemm_rw_kernel``       x, wp, ss_zero (6) + M, K, n_big, mt_out, rot             = 11
* ``gemm_rwr_kernel``      x, wp, ss_zero (6) + M, K, rot                            = 9
* ``gemm_rwk_kernel``      x, wp, ss_zero (6) + M, N, K, S, mt_out, rot              = 12
* ``gemm_lds_kernel``      x, wp, ss_zero (6) + M, N, K, rot                         = 10
* ``gemm_packed_kernel``   x, wp, gate, ss_zero, x_stride (10) + M, N, K, rot        = 14
* ``gemm_sk_kernel``       x, wp, cnt, ss_zero (8) + M, N, K, remap                  = 12
* ``paged_attn1_kernel``   kc, vc, block_tables, q_seq, q_ctx (10) + bt_stride, window, pk_heads, pk_geom = 14
* ``attn_mfma_kernel``     the same 14
* ``splitk_reduce_kernel`` part (2) + M, N + y, ys, res, rs (8) = 12: not reordered, its first loads
  (the slabs and the residual row) were already within the preloaded dwords
"""
import os
import re
import subprocess

import pytest

from src.ops import build as ops_build

LLVM_BIN = "/opt/rocm/llvm/bin"
OBJDUMP = os.path.join(LLVM_BIN, "llvm-objdump")
NEED = {
    "gemm_rw_kernel": 11,
    "gemm_rwr_kernel": 9,
    "gemm_rwk_kernel": 12,
    "gemm_lds_kernel": 10,
    "gemm_packed_kernel": 14,
    "gemm_sk_kernel": 12,
    "paged_attn1_kernel": 14,
    "attn_mfma_kernel": 14,
    "splitk_reduce_kernel": 12,
}
# the instantiations the Llama-2-7B 64-session step runs (profiles/r6ktab): they must be in the library
HEADLINE = ("gemm_rw_kernelILi4ELi6ELi4ELi1ELb1ELb0E", "gemm_rwk_kernelILi4ELi4ELb0ELin1ELb0E",
            "gemm_rwk_kernelILi4ELi6ELb0ELin1ELb0E", "splitk_reduce_kernelILi3ELi4ELb1E",
            "paged_attn1_kernelILi128ELi1ELb1ELi4ELb1ELi4ELb0E")

pytestmark = pytest.mark.skipif(not os.path.isdir(LLVM_BIN), reason="no ROCm LLVM tools on this host")


@pytest.fixture(scope="module")
def preload(tmp_path_factory):
    """{mangled kernel name: kernarg preload length} over every gfx950 code object of the library."""
    lib = ops_build.build()  # (returns at once when the library is current)
    tmp = tmp_path_factory.mktemp("kd")
    os.symlink(lib, tmp / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
    objs = sorted(f for f in os.listdir(tmp) if "amdgcn" in f and ops_build.ARCH in f)
    assert objs, os.listdir(tmp)
    out = {}
    for f in objs:
        txt = subprocess.run([OBJDUMP, "-D", "-j", ".rodata", f], cwd=tmp, check=True, capture_output=True,
                             text=True).stdout
        name = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)\.kd>:", line)
            if m:
                name = m.group(1)
                out[name] = 0  # (the directive is only printed when the length is not zero)
                continue
            m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
            if m and name:
                out[name] = int(m.group(1))
    return out


@pytest.mark.parametrize("family", sorted(NEED))
def test_first_loads_are_preloaded(preload, family):
    got = {k: v for k, v in preload.items() if re.search(r"\d" + family + "I", k)}
    assert got, f"no {family} instantiation in the library"
    short = {k: v for k, v in got.items() if v < NEED[family]}
    print(f"{family}: {len(got)} instantiations, preload length {min(got.values())}..{max(got.values())}, "
          f"needs {NEED[family]}")
    assert not short, f"{family}: preload shorter than {NEED[family]} dwords: {short}"


def test_headline_instantiations_are_present(preload):
    for frag in HEADLINE:
        assert any(frag in k for k in preload), frag


def test_preload_never_exceeds_the_user_sgprs(preload):
    """16 user SGPRs minus the kernarg segment pointer: the rule the argument orders are built on."""
    assert preload and max(preload.values()) <= 14, max(preload.values())
