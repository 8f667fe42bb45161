"""
The one place of the test-suite that calls a host compiler (TEST INFRASTRUCTURE ONLY): the host emulators of tests/emu/ as shared
libraries, stand-alone programs (plain or with AddressSanitizer and UndefinedBehaviorSanitizer), and "include/rfx.h compiles as C99".
Every caller passes its own flags.  The ISA tests drive hipcc themselves.
"""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
INCLUDE = os.path.join(ROOT, "include")
CC, CXX = "gcc", "g++"
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@functools.lru_cache(maxsize=1)
def _tmp():
    d = tempfile.mkdtemp(prefix="rfx_emu_build")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _out(stem):
    return tempfile.mkdtemp(prefix=stem + "_", dir=_tmp())


def src(name):
    """the path of a file of tests/emu/ (an absolute path is returned as it is)"""
    return os.path.join(EMU_DIR, name)


@functools.lru_cache(maxsize=None)
def shared(source, *flags):
    """`g++ -O2 <flags> -shared -fPIC` of one file of tests/emu/: the .so's path, compiled once per (source, flags) and process"""
    so = os.path.join(_out("so"), "lib" + os.path.splitext(os.path.basename(source))[0] + ".so")
    subprocess.run([CXX, "-O2", *flags, "-shared", "-fPIC", "-o", so, src(source)], check=True)
    return so


def program(sources, *flags):
    """a stand-alone executable of the files `sources` (of tests/emu/, or absolute paths; one of them has the main): its path"""
    sources = [sources] if isinstance(sources, str) else list(sources)
    exe = os.path.join(_out("exe"), os.path.splitext(os.path.basename(sources[0]))[0])
    subprocess.run([CXX, *flags, "-o", exe, *[src(str(s)) for s in sources]], check=True)
    return exe


def sanitized_program(sources, *flags, static=True):
    """program() with both sanitizers, their runtimes linked statically unless static=False.  Only ever a program with its own main:
    nothing built here is loaded into Python, and no environment is set."""
    return program(sources, *SANITIZE, *flags, *(("-static-libasan", "-static-libubsan") if static else ()))


def header_compiles_as_c99(tmp_path, body, *, link=False, extra=()):
    """`body` (it includes "rfx.h") compiles as strict C99 with -Wall -Werror -pedantic and the warning flags `extra`; link=True links
    it against librfx.so as a program.  Returns the object's or the program's path."""
    source, out = tmp_path / "use.c", str(tmp_path / ("use" if link else "use.o"))
    source.write_text(body)
    tail = ["-c"]
    if link:
        from riffusion import _hip

        lib_dir = os.path.dirname(_hip.library_path())
        tail = ["-L", lib_dir, "-lrfx", f"-Wl,-rpath,{lib_dir}"]
    subprocess.run([CC, "-std=c99", "-Wall", "-Werror", "-pedantic", *extra, "-I", INCLUDE, str(source), "-o", out, *tail], check=True)
    return out
