"""DevBuf<T> (koifish_amd/host/kf_devbuf.hpp), the host layer's one owner of raw device memory, and the all-or-nothing sets built from it, without a GPU.

tests/devbuf_main.cpp is a stand-alone program: it includes the header, defines the four ABI functions the header calls (kf_malloc, kf_tp_alloc, kf_free, kf_memset) over
host malloc with a record of the live blocks and of the ctx each was allocated with, and refuses the n-th allocation on request -- the out-of-memory paths no device test
can reach.  Built with AddressSanitizer + UBSan and run directly (nothing preloaded): a leak, a double free, a use after free or a free with another ctx fails it.  It
shows: an empty buffer frees nothing; the end of scope leaves no block; Alloc over a held block frees the old one; a failed Alloc leaves the buffer empty; move
construction / assignment transfer, empty the source and free the target's old block, self-move is harmless; every free gets the ctx of its allocation; the uncached form
goes through kf_tp_alloc; and for a two- and a three-member set, with the refusal placed at each member in turn, the held set stays bit for bit what it was, its blocks live."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_devbuf_and_sets_under_sanitizers(tmp_path):
    exe = str(tmp_path / "devbuf_main")
    # the sanitizer runtimes are linked INTO the program: it needs nothing preloaded and does not depend on the order of the libraries a process starts with
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(HERE, "devbuf_main.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert " 0 failed" in run.stdout and " 0 live blocks" in run.stdout and " 0 with another ctx" in run.stdout, run.stdout
