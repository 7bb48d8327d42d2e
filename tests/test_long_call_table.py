"""CPU: what each kind of long-form export hands the engine (csrc/long_call.hpp). tests/cpp/long_call_table.cpp, a program of its
own built with plain g++ under AddressSanitizer + UndefinedBehaviorSanitizer, pushes legacy arguments of every row of the header's
table through the adapters and the one options builder and compares with expectations written out there: whether the options are
null, the number of temperatures, prompted(), per_file_language(), word_timestamps, file_id(1), and every refusal."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_call_table(tmp_path):
    exe = str(tmp_path / "long_call_table")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "whisper.axera_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "long_call_table.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "long_call_table: 0 failures" in r.stdout, r.stdout
