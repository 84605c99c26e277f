#!/usr/bin/env python3
"""Record what the reference's own surface routines compute: tests/golden/heat_faces.npz.

Compiles fistr1/src/lib/heat_LIB_FILM.f90, heat_LIB_RADIATE.f90 and heat_LIB_DFLUX.f90 of the reference tree UNCHANGED (flang -O2,
no default-real-8 switch, as oracle/build_ref.py builds the reference) into a temporary directory together with the small driver
below, which reads elements from a text file and prints, for every face of every element, TERM1, TERM2 and NOD of
heat_FILM_3xx and heat_RADIATE_3xx and VECT of heat_DFLUX_3xx (and VECT of LTYPE = 0, the body flux) with 17 digits.  The three
files `use hecmw` only for the kind parameters; the driver supplies a module of that name with kint and kreal.

    python tests/golden/make_heat_face_golden.py <root of the reference tree>

Per type (341, 342, 351, 352, 361, 362) three skewed elements (frontistr_amd.mesh.solid_mesh plus a random displacement of the
nodes; curved for the quadratic types).  Element 0 has temperatures far above TZERO, element 1 temperatures on both sides of
TZERO (TT - TZERO changes sign across every face), element 2 has TZERO = 0.  Recorded: the inputs and the outputs."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KINDS = """
module hecmw
  integer, parameter :: kint = 4, kreal = 8
end module hecmw
"""


def call(kind, et):
    if kind == "film":
        return "call heat_FILM_%d(nn, XX, YY, ZZ, face, HH, SINK, mm, T1, T2, NOD)" % et
    if kind == "radiate":
        return "call heat_RADIATE_%d(nn, XX, YY, ZZ, TT, face, RR, SINK, TZERO, mm, T1, T2, NOD)" % et
    return "call heat_DFLUX_%d(nn, XX, YY, ZZ, face, Q, VECT)" % et


def select(kind):
    return "      select case (etype)\n" + "".join("      case (%d)\n        %s\n" % (et, call(kind, et)) for et in (341, 342, 351, 352, 361, 362)) + \
        "      end select\n"


MAIN = """
program heat_face
  use m_heat_LIB_FILM
  use m_heat_LIB_RADIATE
  use m_heat_LIB_DFLUX
  implicit none
  integer :: ncase, ic, etype, nn, nface, face, mm, i, NOD(8)
  real(8) :: XX(20), YY(20), ZZ(20), TT(20), T1(64), T2(20), VECT(20), HH, SINK, RR, TZERO, Q
  open(10, file='in.txt', status='old')
  open(11, file='out.txt', status='replace')
  read(10, *) ncase
  do ic = 1, ncase
    read(10, *) etype, nn, nface
    do i = 1, nn
      read(10, *) XX(i), YY(i), ZZ(i), TT(i)
    end do
    read(10, *) HH, SINK, RR, TZERO, Q
    do face = 0, nface
      VECT = 0.d0
%s
      write(11, '(20es26.17e3)') VECT(1:nn)
      if (face == 0) cycle
      mm = 3
      if (etype == 342) mm = 6
      if (etype == 361) mm = 4
      if (etype == 362) mm = 8
      if (etype == 351 .and. face > 2) mm = 4
      if (etype == 352) mm = 8
      if (etype == 352 .and. face < 3) mm = 6
      NOD = 0; T1 = 0.d0; T2 = 0.d0
%s
      write(11, '(9i4)') mm, NOD(1:mm)
      write(11, '(64es26.17e3)') T1(1:mm * mm)
      write(11, '(8es26.17e3)') T2(1:mm)
      NOD = 0; T1 = 0.d0; T2 = 0.d0
%s
      write(11, '(9i4)') mm, NOD(1:mm)
      write(11, '(64es26.17e3)') T1(1:mm * mm)
      write(11, '(8es26.17e3)') T2(1:mm)
    end do
  end do
end program heat_face
""" % (select("dflux"), select("film"), select("radiate"))

HH, SINK, RR, Q = 25.0, 600.0, 1.1164e-8, 2500.0
TZEROS = (-273.15, 400.0, 0.0)


def cases():
    import heat_ref as R
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    rng = np.random.default_rng(20261021)
    out = []
    for et in (341, 342, 351, 352, 361, 362):
        m = CubeMesh(2, skew=0.1) if et == 361 else solid_mesh(2, et, skew=0.1, **({"curve": 0.03} if et in (342, 352, 362) else {}))
        nn = R.NODES[et]
        for k in range(3):
            X = m.coord[m.conn[k * 3 % m.conn.shape[0]] - 1] + 0.02 * rng.standard_normal((nn, 3))
            TT = rng.uniform(300.0, 700.0, nn) if k == 0 else rng.uniform(100.0, 700.0, nn)
            out.append(dict(etype=et, X=X, TT=TT, tzero=TZEROS[k]))
    return out


def main():
    if len(sys.argv) < 2:
        sys.exit("usage: make_heat_face_golden.py <root of the reference tree>")
    ref = sys.argv[1]
    flang = os.environ.get("FLANG", "/opt/rocm/lib/llvm/bin/flang")
    import heat_bc_ref as B
    import heat_ref as R
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "hecmw_kinds.f90"), "w") as f:
            f.write(KINDS)
        with open(os.path.join(tmp, "main.f90"), "w") as f:
            f.write(MAIN)
        lib = os.path.join(ref, "fistr1", "src", "lib")
        subprocess.run([flang, "-O2", "-o", "heat_face", "hecmw_kinds.f90"] +
                       [os.path.join(lib, n) for n in ("heat_LIB_FILM.f90", "heat_LIB_RADIATE.f90", "heat_LIB_DFLUX.f90")] + ["main.f90"],
                       cwd=tmp, check=True)
        with open(os.path.join(tmp, "in.txt"), "w") as f:
            f.write("%d\n" % len(cs))
            for c in cs:
                nn = R.NODES[c["etype"]]
                f.write("%d %d %d\n" % (c["etype"], nn, B.NFACE[c["etype"]]))
                for i in range(nn):
                    f.write(" ".join(repr(float(v)) for v in (*c["X"][i], c["TT"][i])) + "\n")
                f.write(" ".join(repr(float(v)) for v in (HH, SINK, RR, c["tzero"], Q)) + "\n")
        subprocess.run([os.path.join(tmp, "heat_face")], cwd=tmp, check=True)
        lines = iter(open(os.path.join(tmp, "out.txt")).read().split("\n"))
    rec = {"n": np.array(len(cs)), "vals": np.array([HH, SINK, RR, Q])}
    for k, c in enumerate(cs):
        rec["etype%d" % k] = np.array(c["etype"])
        rec["X%d" % k], rec["TT%d" % k], rec["tzero%d" % k] = c["X"], c["TT"], np.array(c["tzero"])
        for face in range(B.NFACE[c["etype"]] + 1):
            rec["dflux%d_%d" % (k, face)] = np.array([float(v) for v in next(lines).split()])
            if face == 0:
                continue
            for kind in ("film", "radiate"):
                head = [int(v) for v in next(lines).split()]
                mm = head[0]
                rec["nod%d_%d" % (k, face)] = np.array(head[1:])
                rec["%s1_%d_%d" % (kind, k, face)] = np.array([float(v) for v in next(lines).split()]).reshape(mm, mm)
                rec["%s2_%d_%d" % (kind, k, face)] = np.array([float(v) for v in next(lines).split()])
    np.savez_compressed(os.path.join(HERE, "heat_faces.npz"), **rec)
    print("wrote heat_faces.npz: %d elements" % len(cs))


if __name__ == "__main__":
    main()
