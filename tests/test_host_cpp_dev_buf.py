"""csrc/dev_buf.h (DevBuf<T>, Workspace) under ASan + UBSan: tests/cpp/dev_buf_host.cpp, a stand-alone program that includes nothing but
the header and supplies the allocator itself -- a counting one that fails the k-th request on demand and records double and foreign
frees.  Run directly (its own process).  The failure paths of the create functions and table caches are tested here and only here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', 'cpp', 'build')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g', '-O1']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')


def test_owners_under_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, 'dev_buf_host')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + SAN + [os.path.join(ROOT, 'tests', 'cpp', 'dev_buf_host.cpp'), '-o', out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and 'dev buf run ok' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]


def test_the_header_includes_no_hip_header():
    text = open(os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd', 'csrc', 'dev_buf.h')).read()
    assert 'hip/' not in text and 'ctx.h' not in text


def test_one_allocator_call_site():
    # the allocator is called in the definitions of dev_alloc / dev_free (capi.hip) and nowhere else under csrc/
    import re
    csrc = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd', 'csrc')
    hits = []
    for name in sorted(n for n in os.listdir(csrc) if n.endswith(('.hip', '.h', '.inc'))):
        for no, line in enumerate(open(os.path.join(csrc, name), errors='replace'), 1):
            code = re.sub(r'"[^"]*"', '""', line.split('//')[0])        # (error labels such as "hipMalloc(tsmon)" and comments do not call it)
            if re.search(r'\bhipMalloc\w*\s*\(|\bhipFree\w*\s*\(|\bbbts_alloc\b|void\* ps\[\]', code):
                hits.append((name, no))
    assert [h[0] for h in hits] == ['capi.hip', 'capi.hip'], hits
