"""The environment in which a child process runs the hipModule form of the library (tests/test_gpu_hipmodule.py, and the stage tests that
run a few of their cases in that form)."""
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MOD_DIR = os.path.join(ROOT, "dabstar_amd", "hipmodule")


def hipmodule_env():
    """os.environ with DABX_LIB and LD_LIBRARY_PATH pointed at hipmodule/libdabx.so, which is built first if it is missing."""
    lib = os.path.join(MOD_DIR, "libdabx.so")
    if not os.path.exists(lib) or not any(f.endswith(".hsaco") for f in os.listdir(MOD_DIR)):
        subprocess.run([sys.executable, "-m", "dabstar_amd.build", "--hipmodule"], check=True, cwd=ROOT, capture_output=True)
    env = dict(os.environ, DABX_LIB=lib)
    env["LD_LIBRARY_PATH"] = MOD_DIR + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    return env
