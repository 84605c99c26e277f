#!/usr/bin/env python3
"""Record what the reference's own element routines compute: tests/golden/heat_elements.npz.

Compiles fistr1/src/lib/heat_LIB_THERMAL.f90 and heat_LIB_CAPACITY.f90 of the reference tree UNCHANGED (flang -O2, no
default-real-8 switch, as oracle/build_ref.py builds the reference) into a temporary directory together with the small driver
below, which reads elements from a text file and prints heat_THERMAL_3xx's SS and heat_CAPACITY_3xx's S0 with 17 digits.  The
two files `use hecmw` only for the kind parameters; the driver supplies a module of that name with kint and kreal.

    python tests/golden/make_heat_elem_golden.py <root of the reference tree>

Per type (341, 342, 351, 352, 361, 362) three skewed elements (frontistr_amd.mesh.solid_mesh, plus a random displacement of the
nodes), node temperatures that put quadrature points in every table interval and on a breakpoint, a conductivity table of three
rows and one of a single row, specific heat and density tables of two rows.  Recorded: the inputs and the outputs."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DRIVER = """
module hecmw
  integer, parameter :: kint = 4, kreal = 8
end module hecmw
program heat_elem
  use m_heat_lib_thermal
  use m_heat_LIB_CAPACITY
  implicit none
  integer :: ncase, ic, etype, nn, i, nt(3)
  real(8) :: XX(20), YY(20), ZZ(20), TT(20), T0(20), SS(400), S0(20)
  real(8) :: temp(10, 3), fA(11, 3), fB(11, 3)
  open(10, file='in.txt', status='old')
  open(11, file='out.txt', status='replace')
  read(10, *) ncase
  do ic = 1, ncase
    read(10, *) etype, nn
    do i = 1, nn
      read(10, *) XX(i), YY(i), ZZ(i), TT(i), T0(i)
    end do
    temp = 0.d0; fA = 0.d0; fB = 0.d0
    do i = 1, 3
      read(10, *) nt(i)
      read(10, *) temp(1:nt(i), i)
      read(10, *) fA(1:nt(i) + 1, i)
      read(10, *) fB(1:nt(i) + 1, i)
    end do
    SS = 0.d0
    S0 = 0.d0
    select case (etype)
    case (341)
      call heat_THERMAL_341(nn, XX, YY, ZZ, TT, 1, SS, nt(1), temp(:, 1), fA(:, 1), fB(:, 1))
      call heat_CAPACITY_341(nn, XX, YY, ZZ, T0, 1, S0, nt(2), temp(:, 2), fA(:, 2), fB(:, 2), nt(3), temp(:, 3), fA(:, 3), fB(:, 3))
    case (342)
      call heat_THERMAL_342(nn, XX, YY, ZZ, TT, 1, SS, nt(1), temp(:, 1), fA(:, 1), fB(:, 1))
      call heat_CAPACITY_342(nn, XX, YY, ZZ, T0, 1, S0, nt(2), temp(:, 2), fA(:, 2), fB(:, 2), nt(3), temp(:, 3), fA(:, 3), fB(:, 3))
    case (351)
      call heat_THERMAL_351(nn, XX, YY, ZZ, TT, 1, SS, nt(1), temp(:, 1), fA(:, 1), fB(:, 1))
      call heat_CAPACITY_351(nn, XX, YY, ZZ, T0, 1, S0, nt(2), temp(:, 2), fA(:, 2), fB(:, 2), nt(3), temp(:, 3), fA(:, 3), fB(:, 3))
    case (352)
      call heat_THERMAL_352(nn, XX, YY, ZZ, TT, 1, SS, nt(1), temp(:, 1), fA(:, 1), fB(:, 1))
      call heat_CAPACITY_352(nn, XX, YY, ZZ, T0, 1, S0, nt(2), temp(:, 2), fA(:, 2), fB(:, 2), nt(3), temp(:, 3), fA(:, 3), fB(:, 3))
    case (361)
      call heat_THERMAL_361(nn, XX, YY, ZZ, TT, 1, SS, nt(1), temp(:, 1), fA(:, 1), fB(:, 1))
      call heat_CAPACITY_361(nn, XX, YY, ZZ, T0, 1, S0, nt(2), temp(:, 2), fA(:, 2), fB(:, 2), nt(3), temp(:, 3), fA(:, 3), fB(:, 3))
    case (362)
      call heat_THERMAL_362(nn, XX, YY, ZZ, TT, 1, SS, nt(1), temp(:, 1), fA(:, 1), fB(:, 1))
      call heat_CAPACITY_362(nn, XX, YY, ZZ, T0, 1, S0, nt(2), temp(:, 2), fA(:, 2), fB(:, 2), nt(3), temp(:, 3), fA(:, 3), fB(:, 3))
    end select
    write(11, '(400es26.17e3)') SS(1:nn * nn)
    write(11, '(20es26.17e3)') S0(1:nn)
  end do
end program heat_elem
"""

COND3 = [(50.0, 0.0), (42.0, 200.0), (35.0, 500.0)]
COND1 = [(50.0, 0.0)]
CP2 = [(0.46, 0.0), (0.52, 400.0)]
RHO2 = [(7.85, 0.0), (7.70, 400.0)]


def cases():
    import heat_ref as R
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    rng = np.random.default_rng(20261020)
    out = []
    for et in (341, 342, 351, 352, 361, 362):
        m = CubeMesh(2, skew=0.1) if et == 361 else solid_mesh(2, et, skew=0.1, **({"curve": 0.03} if et in (342, 352, 362) else {}))
        nn = R.NODES[et]
        for k, cond in enumerate((COND3, COND3, COND1)):
            X = m.coord[m.conn[k * 3 % m.conn.shape[0]] - 1] + 0.02 * rng.standard_normal((nn, 3))
            # below the first row, inside both intervals, above the last row; one element exactly on the breakpoint 200
            TT = rng.uniform(-150.0, 700.0, nn) if k != 1 else np.full(nn, 200.0)
            T0 = rng.uniform(-100.0, 600.0, nn) if k != 1 else np.full(nn, 400.0)
            out.append(dict(etype=et, X=X, TT=TT, T0=T0, cond=cond))
    return out


def main():
    if len(sys.argv) < 2:
        sys.exit("usage: make_heat_elem_golden.py <root of the reference tree>")
    ref = sys.argv[1]
    flang = os.environ.get("FLANG", "/opt/rocm/lib/llvm/bin/flang")
    import heat_ref as R
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.f90"), "w") as f:
            f.write(DRIVER)
        # module hecmw comes first: split the driver's module into its own file
        with open(os.path.join(tmp, "hecmw_kinds.f90"), "w") as f:
            f.write(DRIVER.split("program heat_elem")[0])
        with open(os.path.join(tmp, "main.f90"), "w") as f:
            f.write("program heat_elem" + DRIVER.split("program heat_elem", 1)[1])
        lib = os.path.join(ref, "fistr1", "src", "lib")
        subprocess.run([flang, "-O2", "-o", "heat_elem", "hecmw_kinds.f90", os.path.join(lib, "heat_LIB_THERMAL.f90"),
                        os.path.join(lib, "heat_LIB_CAPACITY.f90"), "main.f90"], cwd=tmp, check=True)
        with open(os.path.join(tmp, "in.txt"), "w") as f:
            f.write("%d\n" % len(cs))
            for c in cs:
                nn = R.NODES[c["etype"]]
                f.write("%d %d\n" % (c["etype"], nn))
                for i in range(nn):
                    f.write(" ".join(repr(float(v)) for v in (*c["X"][i], c["TT"][i], c["T0"][i])) + "\n")
                for rows in (c["cond"], CP2, RHO2):
                    n, temp, fA, fB = R.make_table(rows)
                    f.write("%d\n%s\n%s\n%s\n" % (n, " ".join(repr(float(v)) for v in temp), " ".join(repr(float(v)) for v in fA),
                                                  " ".join(repr(float(v)) for v in fB)))
        subprocess.run([os.path.join(tmp, "heat_elem")], cwd=tmp, check=True)
        vals = open(os.path.join(tmp, "out.txt")).read().split("\n")
    rec = {"n": np.array(len(cs))}
    for k, c in enumerate(cs):
        nn = R.NODES[c["etype"]]
        rec["etype%d" % k] = np.array(c["etype"])
        rec["X%d" % k], rec["TT%d" % k], rec["T0%d" % k] = c["X"], c["TT"], c["T0"]
        rec["cond%d" % k] = np.array(c["cond"])
        rec["SS%d" % k] = np.array([float(v) for v in vals[2 * k].split()]).reshape(nn, nn)
        rec["S0%d" % k] = np.array([float(v) for v in vals[2 * k + 1].split()])
    rec["cp"], rec["rho"] = np.array(CP2), np.array(RHO2)
    np.savez_compressed(os.path.join(HERE, "heat_elements.npz"), **rec)
    print("wrote heat_elements.npz: %d elements" % len(cs))


if __name__ == "__main__":
    main()
