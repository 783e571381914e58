"""What the CPU tests of the side libraries (libbhnerf_kerr.so, libbhnerf_eht.so, libbhnerf_grf.so) share: the sanitizer build of a
stand-alone host program of tools/, the run of it as a child process, and the conventions every side library is held to.  Imported
by the tests the way gr_factor_cases.py is; nothing built with a sanitizer is loaded into the Python process."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# public header, and the names of its library's path and ctypes table in bhnerf_amd/_hip.py
LIBRARIES = (('bhnerf_hip.h', 'LIB_PATH', 'SIGNATURES'), ('bhnerf_kerr.h', 'KERR_LIB_PATH', 'KERR_SIGNATURES'),
             ('bhnerf_eht.h', 'EHT_LIB_PATH', 'EHT_SIGNATURES'), ('bhnerf_grf.h', 'GRF_LIB_PATH', 'GRF_SIGNATURES'))
BANNED = ('hipMalloc', 'hipFree', 'hipHostMalloc', 'getenv', 'hipStreamSynchronize', 'hipDeviceSynchronize', 'malloc')


def build_host_program(tmp_path_factory, name):
    """tools/<name>.cpp built with g++, AddressSanitizer and UBSan in a fresh directory -> (exe, that directory)."""
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed to build tools/%s.cpp' % name
    work = tmp_path_factory.mktemp(name)
    exe = str(work / name)
    cmd = [gxx, '-O2', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall',
           '-I', os.path.join(ROOT, 'bhnerf_amd', 'csrc'), os.path.join(ROOT, 'tools', name + '.cpp'), '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe, work


def run_host(exe, *args):
    """The program as a child process on its arguments (the input and the output file): it must exit 0 and report nothing."""
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
    assert not res.stderr.strip(), res.stderr[-4000:]           # a sanitizer report


def _header(name):
    text = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def _symbols(path, which):
    nm = shutil.which('nm')
    assert nm, 'nm is needed to read the symbol table'
    return subprocess.run([nm, '-D', which, path], capture_output=True, text=True, check=True).stdout


def assert_library_conventions(header, lib_path, signatures, prefix, expected_names):
    """The dynamic symbol table of the library is the declarations of include/<header> and nothing else, the ctypes table binds
    exactly those, and the library references no allocator, no getenv and no synchronisation (the conventions of
    include/bhnerf_hip.h, which tests/test_abi_cpu.py holds libbhnerf_hip.so to).  The other three libraries, their headers and
    their ctypes tables do not know a name that begins with `prefix`."""
    import __graft_entry__ as entry
    entry.build()
    from bhnerf_amd import _hip
    declared = sorted(set(re.findall(r'\b(bhn_\w+)\s*\(', _header(header))))
    assert declared == sorted(signatures) == sorted(expected_names)
    assert sorted(line.split()[-1] for line in _symbols(lib_path, '--defined-only').splitlines() if line.strip()) == declared
    undefined = _symbols(lib_path, '--undefined-only')
    for banned in BANNED:
        assert banned not in undefined, banned
    others = [(h, getattr(_hip, p), getattr(_hip, t)) for h, p, t in LIBRARIES if h != header]
    assert len(others) == len(LIBRARIES) - 1 == 3
    for other_header, path, table in others:
        assert prefix not in _header(other_header), other_header
        assert prefix not in _symbols(path, '--defined-only'), path
        assert not any(k.startswith(prefix) for k in table), other_header
