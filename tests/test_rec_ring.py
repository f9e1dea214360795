"""csrc/rec_ring.h, the one statement of which records a reader of a record ring takes (the dabx_read_* entries of the TII, scope, CIR and
spectrum stages, and their sections of the bulk delivery): tests/cxx/rec_ring_check.cpp includes it with plain g++, without HIP, and checks
the window function against a brute-force model over every total in 0..40, every cursor up to it and beyond, and every ring length and
chunk share the library uses.  Built twice: as it is, and with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(__file__), "..")


@pytest.mark.parametrize("exe", ["rec_ring_check", "rec_ring_check_san"])
def test_record_window_matches_its_brute_force_model(exe):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cxx"), "recring"], check=True)
    p = subprocess.run([os.path.join(ROOT, "tests", "cxx", "_build", exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "rec_ring_check ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
