"""The only hand-written threading of the library -- the per-device workers of a sharded handle that lists several devices,
csrc/fir_shard_workers.h -- without a GPU: tests/shard_workers_main.cpp, a stand-alone program, is built with the host compiler
under the thread sanitizer and under the address / undefined-behaviour sanitizers, and each binary is run directly. Nothing is
loaded into Python. The program checks, for 1, 2 and 8 slots: every job once per round on its slot's own thread, the lowest
failing slot's code and text, search_host's handshake in both orders of arrival, and teardown in every state."""
import os
import platform
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-image-recognition_amd", "csrc")
NO_SHADOW = "unexpected memory mapping"     # the thread sanitizer's runtime gave up before main(): nothing of the program ran


def build(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    static = []
    if "clang" not in os.path.basename(cxx):      # (clang links the runtimes statically by itself)
        static = [lib for word, lib in (("thread", "-static-libtsan"), ("address", "-static-libasan"), ("undefined", "-static-libubsan"))
                  if word in " ".join(flags)]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", *flags, *static, "-I", CSRC,
                    os.path.join(ROOT, "tests", "shard_workers_main.cpp"), "-o", exe], check=True)
    return exe


def passes(exe, prefix=()):
    run = subprocess.run([*prefix, exe], capture_output=True, text=True)
    if NO_SHADOW in run.stderr:
        return False
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert run.stdout.splitlines() == ["slots 1 ok", "slots 2 ok", "slots 8 ok", "ok"]
    return True


def test_the_worker_threads_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    assert passes(build(tmp_path, "workers_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_the_worker_threads_under_the_thread_sanitizer(tmp_path):
    """Older thread-sanitizer runtimes cannot place their shadow memory where a kernel randomises mappings over more than 28 bits
    and stop before main(). Address-space randomisation is a flag of the process: the program is then started once more without
    it (setarch -R). Where the runtime cannot start even so, the program's own assertions still run, without the sanitizer."""
    exe = build(tmp_path, "workers_tsan", ["-fsanitize=thread", "-fno-sanitize-recover=all"])
    if passes(exe):
        return
    if shutil.which("setarch") and passes(exe, ("setarch", platform.machine(), "-R")):
        return
    print("the thread sanitizer cannot start on this machine: plain assertions only")
    assert passes(build(tmp_path, "workers_plain", []))
