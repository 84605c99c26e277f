"""`--lib PATH` of the benchmark scripts: time another build of libfistr_hip.so (the parent commit's, say) with the same script."""
import os
import sys

from frontistr_amd import hecmw as hip


def take_lib(argv=sys.argv):
    """Removes `--lib PATH` from argv and makes PATH the library hecmw.lib() loads; returns the path in use."""
    if "--lib" in argv:
        k = argv.index("--lib")
        if k + 1 >= len(argv):
            sys.exit("--lib needs the path of a libfistr_hip.so")
        hip.LIBPATH = os.path.abspath(argv[k + 1])
        del argv[k:k + 2]
    return hip.LIBPATH
