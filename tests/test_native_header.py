"""CPU: the reader that derives the ctypes binding from include/u3d.h (pytorch3dunet_amd/_native.py: `parse_header`) — what it accepts
on small synthetic headers, that everything it does not understand raises instead of being skipped, and the derived structure classes
against the layout the host C compiler gives the real header."""
import ctypes
import os
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

import pytest

from conftest import ROOT
from pytorch3dunet_amd import _native as nat

GOOD = """
/* u3d_foo(int a); in a comment is no declaration, nor is
 * int u3d_bar(void); on a continuation line */
#ifndef U3D_H
#define U3D_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_VERSION 7 /* 7: u3d_baz( added */
#define U3D_EINVAL (-1)
typedef void* u3d_stream_t; /* hipStream_t */
typedef struct {
    const float* p0; /* u3d_in_a_field_comment( */
    int32_t C0, C1;
    int64_t first;
    double count;
    float scale;
} u3d_a_t;
typedef struct u3d_b {
    const double* lo;
    int32_t N, G, reserved;
} u3d_b_t;
int u3d_version(void);
int u3d_nothing();
const char* u3d_last_error(void);
// u3d_line_comment(int a);
size_t u3d_three_lines(int device, u3d_stream_t stream, const u3d_a_t* src,
                       const float* w, float* out, long long n, int64_t m,
                       double eps, float slope, const u3d_b_t* job, uint8_t* argmax);
long long u3d_box(int device, const int* box, const int32_t* zlo, void* buf, size_t bytes);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reads_declarations_structs_and_constants():
    protos, structs, consts = nat.parse_header(GOOD)
    assert list(protos) == ["u3d_version", "u3d_nothing", "u3d_last_error", "u3d_three_lines", "u3d_box"]  # header order, comments ignored
    assert protos["u3d_version"] == (c_int, []) and protos["u3d_nothing"] == (c_int, [])  # `(void)` and `()`
    assert protos["u3d_last_error"] == (c_char_p, [])  # a `const char*` return
    assert protos["u3d_three_lines"] == (c_size_t, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_double, c_float,
                                                     c_void_p, c_void_p])  # a declaration broken over three lines
    assert protos["u3d_box"] == (c_int64, [c_int, c_void_p, c_void_p, c_void_p, c_size_t])  # `const int* box`: an array is a pointer
    assert list(structs) == ["u3d_a_t", "u3d_b_t"]  # without and with a tag
    assert structs["u3d_a_t"] == [("p0", c_void_p), ("C0", c_int32), ("C1", c_int32), ("first", c_int64), ("count", c_double),
                                  ("scale", c_float)]
    assert structs["u3d_b_t"] == [("lo", c_void_p), ("N", c_int32), ("G", c_int32), ("reserved", c_int32)]
    assert consts == {"U3D_VERSION": 7, "U3D_EINVAL": -1}


def test_a_header_without_the_extern_c_wrapper_reads_the_same():
    assert nat.parse_header("int u3d_a(int x);\nfloat u3d_b(const float* p);")[0] == {"u3d_a": (c_int, [c_int]), "u3d_b": (c_float, [c_void_p])}


@pytest.mark.parametrize("text,named", [
    ("int u3d_a(unsigned short x);", "unsigned short"),                      # a type token that is not in the table ...
    ("int u3d_a(int x, wchar_t* s);", "wchar_t*"),                           # ... also behind a pointer
    ("unsigned u3d_a(int x);", "u3d_a"),                                     # ... and as a return type
    ("float* u3d_a(int x);", "u3d_a"),
    ("int u3d_a(int);", "u3d_a"),                                            # an argument without a name
    ("int u3d_ok(int x);\nstatic inline int u3d_x (int a) { return a; }", "u3d_x ("),  # a `u3d_*(` that was not consumed as a declaration
    ("int u3d_ok(int x);\nint u3d_cb(int (*fn)(int));", "u3d_cb("),
    ("int u3d_ok(int x)\nint u3d_b(int y);", "u3d_ok"),                      # a missing semicolon swallows the next declaration
    ("int u3d_a(int x);\nint u3d_a(int x);", "u3d_a is declared twice"),    # a name declared twice
    ("typedef struct { int32_t a; } u3d_s_t;\ntypedef struct { int32_t a; } u3d_s_t;", "u3d_s_t is declared twice"),
    ("typedef struct { unsigned a; } u3d_s_t;", "struct u3d_s_t"),           # struct fields that do not parse
    ("typedef struct { int32_t a[4]; } u3d_s_t;", "struct u3d_s_t"),
    ("typedef struct { float *a, *b; } u3d_s_t;", "struct u3d_s_t"),
    ("typedef struct { int32_t a : 3; } u3d_s_t;", "struct u3d_s_t"),
    ("typedef struct { struct { int32_t a; } in; } u3d_s_t;", "typedef struct"),  # nested braces: not consumed
    ("typedef int u3d_index_t;\nint u3d_a(int x);", "typedef int"),         # anything else left over
    ("#define U3D_VERSION (127 + 1)\nint u3d_a(int x);", "U3D_VERSION"),    # a constant that is not one integer
    ("#define U3D_OK 0\n#define U3D_OK 0\n", "U3D_OK"),
    ("#define U3D_CALL(x) u3d_##x\nint u3d_a(int x);", "U3D_CALL"),          # preprocessor lines other than the header's own kinds
    ("#define int long\nint u3d_a(int x);", "define int long"),
    ("#if 0\nint u3d_a(int x);\n#endif", "#if 0"),
    ("#ifdef U3D_EXTRAS\nint u3d_a(int x);\n#endif", "U3D_EXTRAS"),
])
def test_what_it_does_not_understand_raises(text, named):
    with pytest.raises(nat.U3DError) as e:
        nat.parse_header(text)
    assert named in str(e.value), str(e.value)


def test_missing_header_says_where_it_looked(tmp_path):
    path = str(tmp_path / "include" / "u3d.h")
    with pytest.raises(nat.U3DError) as e:
        nat.read_header(path)
    assert path in str(e.value) and "include/u3d.h" in str(e.value)


def test_a_header_that_lacks_a_named_struct_or_constant_raises(tmp_path):
    path = tmp_path / "u3d.h"
    path.write_text(GOOD)
    with pytest.raises(nat.U3DError):
        nat.read_header(str(path))


def test_the_real_header_is_the_binding():
    assert nat.HEADER_PATH == os.path.join(ROOT, "include", "u3d.h")
    protos, structs, consts = nat.read_header(nat.HEADER_PATH)
    assert protos == nat._PROTOS and list(protos) == list(nat.EXPORTED_SYMBOLS) and len(protos) == 250
    assert (nat.U3D_VERSION, nat.U3D_OK, nat.U3D_EINVAL, nat.U3D_EHIP, nat.U3D_EARCH, nat.U3D_EWORKSPACE) == (128, 0, -1, -2, -3, -4)
    for cname, cls in (("u3d_src_t", nat.U3DSrc), ("u3d_adam_desc_t", nat.U3DAdamDesc), ("u3d_gn_bwd_job_t", nat.U3DGnBwdJob),
                       ("u3d_pack_desc_t", nat.U3DPackDesc)):
        assert issubclass(cls, ctypes.Structure) and cls._fields_ == structs[cname]
    # every pointer is c_void_p, whatever it points to: the forms the call sites pass all convert
    void_p = nat._PROTOS["u3d_conv3d_box"][1]
    assert void_p[2] is c_void_p and void_p[-1] is c_void_p and void_p[-2] is c_void_p
    for arg in (ctypes.byref(nat.U3DSrc()), (ctypes.c_int * 6)(1, 2, 3, 4, 5, 6), ctypes.byref(ctypes.c_double()), 1 << 40, None):
        c_void_p.from_param(arg)


_STRUCTS = {"u3d_src_t": "U3DSrc", "u3d_adam_desc_t": "U3DAdamDesc", "u3d_gn_bwd_job_t": "U3DGnBwdJob", "u3d_pack_desc_t": "U3DPackDesc"}


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof of the four structs, printed by a C program that includes u3d.h, against the derived classes"""
    cc = shutil.which(os.environ.get("CC", "gcc"))  # the host C compiler of oracle/Makefile
    if cc is None:
        pytest.skip("no host C compiler (CC / gcc) found")
    lines = []
    for cname, py in _STRUCTS.items():
        lines.append(f'    printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in getattr(nat, py)._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "u3d.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True, capture_output=True, timeout=60)
    got = [tuple(l.split()) for l in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()]
    want = []
    for cname, py in _STRUCTS.items():
        cls = getattr(nat, py)
        want.append((cname, "sizeof", str(ctypes.sizeof(cls))))
        want += [(cname, f, str(getattr(cls, f).offset)) for f, _ in cls._fields_]
    assert got == want and len(got) == 4 + 11 + 6 + 17 + 7
