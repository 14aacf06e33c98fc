"""CPU: the four ownership types of the library's host side (csrc/owned.h: DevBuf, PinnedBuf, Event, Stream) before they reach a GPU. The header,
and nothing else of the library, is compiled with g++ under AddressSanitizer + UBSan into a stand-alone program (tests/owned_host.cpp) that is NOT
linked against the HIP runtime: it defines the nine HIP functions the header calls itself, over malloc, with their own count of what is live and
a switch that fails the k-th acquisition. Every scenario compares the handles' live counters (what ctpn_debug_live_resources reports) with the
fakes' own count; a release of something not live aborts, and the leak check runs at exit."""
import os
import subprocess

import pytest

SCENARIOS = ["moves", "grow", "grow_fail", "grow_retiring_fail", "grow_retiring_ok", "kth_failure", "pair_retry", "event_ensure", "exit"]


@pytest.fixture(scope="module")
def run(root, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("owned") / "owned_host")
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(root, "tests", "owned_host.cpp")], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_the_program_is_clean_under_the_sanitizers(run):
    assert "AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert [line.split()[1] for line in run.stdout.splitlines()] == SCENARIOS


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario(run, name):
    """moves: move construction / assignment leave the source empty and release the target's old resource once, for all four types.
    grow: below, at and above the size. grow_fail: a failed grow leaves {null, 0} with the old block released.
    grow_retiring_fail: the old block stays, `retired` unchanged. grow_retiring_ok: the old block moves into `retired` and its pointer stays
    valid until the vector dies. kth_failure: a struct of several handles whose k-th acquisition fails, for every k, ends with nothing live.
    pair_retry: a page-locked block and its device twin, each tested against the need on its own (the device Huffman decoder's staging pair): a
    call in which one grew and the twin could not is completed by the next call of the same size. event_ensure: ensure twice creates once. exit: every counter zero at exit."""
    lines = [line for line in run.stdout.splitlines() if line.split()[:2] == ["ok", name]]
    assert len(lines) == 1, (run.stdout[-2000:], run.stderr[-2000:])
    if name == "kth_failure":
        assert int(lines[0].split()[2]) == 15      # the acquisitions of the struct: each one was failed once
    if name == "exit":
        t = lines[0].split()
        assert int(t[3]) > 0 and int(t[5]) > 0 and int(t[3]) - int(t[5]) == 15 + 8      # every acquisition that succeeded was released: 15 + 8 were refused
