"""The g++ builds of the host-compilable headers of dicp_amd/csrc (tests/hostcheck/*.cpp), for the CPU tests.

A plain module (no fixtures): the tests put this directory on sys.path and import it.
"""
import ctypes
import glob
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTCHECK = os.path.join(HERE, "hostcheck")
FLAGS = ["-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas"]


def build(src, name, extra_flags=()):
    """g++ FLAGS + extra_flags on tests/hostcheck/<src> -> CDLL of tests/hostcheck/lib<name>.so, rebuilt when the source or a header of
    dicp_amd/csrc is newer (one name per set of flags).  Skips the calling test without g++."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src, lib = os.path.join(HOSTCHECK, src), os.path.join(HOSTCHECK, "lib%s.so" % name)
    deps = [src, os.path.abspath(__file__)] + glob.glob(os.path.join(HERE, "..", "dicp_amd", "csrc", "*.h"))
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in deps):
        tmp = "%s.%d.tmp" % (lib, os.getpid())
        subprocess.check_call(["g++"] + FLAGS + list(extra_flags) + ["-o", tmp, src])
        os.replace(tmp, lib)
    return ctypes.CDLL(lib)
