"""The host-only index tables of the region layer (csrc/include_internal/host_tables.h): the CSR builder and the river
network tables, and the calendar tables of pt_gs_k (build_year_tables: day of year and time since New Year of every
step, against a day-by-day walk over the axes of tests/time_axis_cases.py and whole years around 1900, 1970, 2000, 2016,
2100 and 2400), checked by tools/host_tables_check.cpp under the address and undefined-behaviour sanitizers. The
program is built and run as a child process on the CPU; nothing of it is loaded into this interpreter."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_host_tables_under_sanitizers(tmp_path):
    exe = tmp_path / "host_tables_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tools" / "host_tables_check.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks passed" in run.stdout
