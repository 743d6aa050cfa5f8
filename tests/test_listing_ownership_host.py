"""Who owns what the string layer's six key-listing calls hand out (rio_op_snapshot, rio_op_objects_on_server, rio_op_rebalance,
rio_op_changes, rio_op_expire, rio_op_hottest_objects), without a GPU: the arrays are the calling thread's until its next call
of the SAME function.  tests/host_layer_listing_driver.cpp holds a listing of each, calls everything else on the same thread and
the same function on another, and reads the listing again; it is built with AddressSanitizer, so a string that was freed or
moved meanwhile fails the run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread", "-I", os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    """The string layer and the driver, compiled once for both programs."""
    d = tmp_path_factory.mktemp("listing_driver")
    out = []
    for src in (os.path.join(ROOT, "rio-rs_amd", "csrc", "gpu_object_placement.cpp"),
                os.path.join(ROOT, "tests", "host_layer_listing_driver.cpp")):
        out.append(str(d / (os.path.basename(src) + ".o")))
        subprocess.run(FLAGS + ["-c", src, "-o", out[-1]], check=True)
    return d, out


def _run(objects, stub, args):
    d, objs = objects
    exe = d / ("driver_" + os.path.splitext(stub)[0])
    subprocess.run(FLAGS + objs + [os.path.join(ROOT, "tests", stub), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "runtime error:" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "wrong=0" in r.stdout


def test_a_listing_survives_every_other_call_and_other_threads(objects):
    """Checks A, B, C and D's refused call, over the stub that has all six dense calls."""
    _run(objects, "stub_rio_gp_listing.cpp", [])


def test_a_call_the_dense_layer_lacks_lists_nothing(objects):
    """Check D's RIO_GP_EUPSTREAM: rio_op_expire over the plain stub sets *n_out = 0; a snapshot after it lists every key."""
    _run(objects, "stub_rio_gp.cpp", ["plain"])
