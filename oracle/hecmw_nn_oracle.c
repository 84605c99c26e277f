/* TEST INFRASTRUCTURE ONLY -- part of the CPU oracle (included by hecmw_oracle.c).
 *
 * Block sizes other than 3: restatement of the reference's generic-NDOF routines
 *   hecmw_matvec_nn_inner        hecmw1/src/solver/las/hecmw_solver_las_nn.f90:135-310
 *   hecmw_precond_DIAG_nn_*      hecmw1/src/solver/precond/nn/hecmw_precond_DIAG_nn.f90:27-137
 *   hecmw_precond_SSOR_nn_*      hecmw1/src/solver/precond/nn/hecmw_precond_SSOR_nn.f90:55-213 (setup), :215-420 (apply)
 *   FORM_ILU0_nn / BILU_nn_apply hecmw1/src/solver/precond/nn/hecmw_precond_BILU_nn.f90:196-333, :90-168 (NDOF = 5; the
 *                                unrolled FORM_ILU0_44 / _66 and BILU_44 / _66 apply of precond/44, precond/66 for 4 and 6)
 * The reference dispatches NDOF = 1, 2, 4, 6 to hand-unrolled copies (las_11/22/44/66, precond/11/22/44/66) of the
 * same loops -- same LU without pivoting, same sweep order -- so one restatement covers them to rounding; the parity
 * tests pin it against the real reference for NDOF = 1, 2, 4, 5 (the true _nn path) and 6.
 * The Krylov loops themselves are NDOF-generic in the reference (hecmw_solver_CG.f90 etc.) and in hecmw_oracle.c. */

void orc_matvec_nn(const orc_matrix *A, const orc_comm *c, double *X, double *Y) {
  const int nd = ORC_ND(A), nd2 = nd * nd;
  const int32_t N = A->N;
  double XV[16], YV[16];
  if (c && c->halo) c->halo(X, c->ctx); /* hecmw_update_m_R :247 */
  for (int32_t i = 1; i <= N; i++) { /* :269-312 */
    for (int k = 0; k < nd; k++) { XV[k] = X[(size_t)nd * (i - 1) + k]; YV[k] = 0.0; }
    for (int k = 0; k < nd; k++)
      for (int l = 0; l < nd; l++) YV[k] = YV[k] + A->D[(size_t)nd2 * (i - 1) + k * nd + l] * XV[l];
    for (int32_t j = A->indexL[i - 1] + 1; j <= A->indexL[i]; j++) {
      const int32_t in = F1(A->itemL, j);
      for (int k = 0; k < nd; k++) XV[k] = X[(size_t)nd * (in - 1) + k];
      for (int k = 0; k < nd; k++)
        for (int l = 0; l < nd; l++) YV[k] = YV[k] + A->AL[(size_t)nd2 * (j - 1) + k * nd + l] * XV[l];
    }
    for (int32_t j = A->indexU[i - 1] + 1; j <= A->indexU[i]; j++) {
      const int32_t in = F1(A->itemU, j);
      for (int k = 0; k < nd; k++) XV[k] = X[(size_t)nd * (in - 1) + k];
      for (int k = 0; k < nd; k++)
        for (int l = 0; l < nd; l++) YV[k] = YV[k] + A->AU[(size_t)nd2 * (j - 1) + k * nd + l] * XV[l];
    }
    for (int k = 0; k < nd; k++) Y[(size_t)nd * (i - 1) + k] = YV[k];
  }
}

/* LU without pivoting, reciprocal pivots on the diagonal: DIAG_nn.f90:80-91 == SSOR_nn.f90:186-197.  a: row-major nd x nd */
static void lu_nn(int nd, double *a, double SIGMA_DIAG) {
  double PW[16];
  for (int i = 0; i < nd; i++) a[i * nd + i] = a[i * nd + i] * SIGMA_DIAG;
  for (int k = 0; k < nd; k++) {
    a[k * nd + k] = 1.0 / a[k * nd + k];
    for (int i = k + 1; i < nd; i++) {
      a[i * nd + k] = a[i * nd + k] * a[k * nd + k];
      for (int j = k + 1; j < nd; j++) PW[j] = a[i * nd + j] - a[i * nd + k] * a[k * nd + j];
      for (int j = k + 1; j < nd; j++) a[i * nd + j] = PW[j];
    }
  }
}

/* forward / back substitution with the block of lu_nn: DIAG_nn.f90:111-121 == SSOR_nn.f90:321-331.
 * quirk66: the hand-unrolled NDOF = 6 SSOR of the reference (precond/66/hecmw_precond_SSOR_66.f90:420 and :504) reads
 * ALU(36*i-5) = entry (6,1) where entry (4,3) = ALU(36*i-15) belongs, in both sweeps; DIAG_66 does not.  The reference's
 * results (iteration counts included) carry that, so the restatement reproduces it. */
static void lusolve_nn_q(int nd, const double *alu, double *X, int quirk66) {
  for (int j = 1; j < nd; j++)
    for (int k = 0; k < j; k++) X[j] = X[j] - ((quirk66 && j == 3 && k == 2) ? alu[nd * 5] : alu[nd * j + k]) * X[k];
  for (int j = nd - 1; j >= 0; j--) {
    for (int k = nd - 1; k > j; k--) X[j] = X[j] - alu[nd * j + k] * X[k];
    X[j] = alu[(nd + 1) * j] * X[j];
  }
}
static void lusolve_nn(int nd, const double *alu, double *X) { lusolve_nn_q(nd, alu, X, 0); }

static void diag_nn_setup(orc_precond *P, const orc_matrix *A, double SIGMA_DIAG) {
  const int nd = P->ndof, nd2 = nd * nd;
  P->ALU = (double *)calloc((size_t)nd2 * A->NP, sizeof(double));
  memcpy(P->ALU, A->D, (size_t)nd2 * A->N * sizeof(double));
  for (int32_t ii = 0; ii < A->N; ii++) lu_nn(nd, &P->ALU[(size_t)nd2 * ii], SIGMA_DIAG);
}

static void diag_nn_apply(const orc_precond *P, double *WW) {
  const int nd = P->ndof;
  for (int32_t i = 0; i < P->N; i++) lusolve_nn(nd, &P->ALU[(size_t)nd * nd * i], &WW[(size_t)nd * i]);
}

static void reorder_profile(int32_t N, const int32_t *perm, const int32_t *iperm, const int32_t *indexL,
                            const int32_t *indexU, const int32_t *itemL, const int32_t *itemU, int32_t *indexLp,
                            int32_t *indexUp, int32_t *itemLp, int32_t *itemUp);
static int32_t bsearch_1(const int32_t *array, int32_t istart, int32_t iend, int32_t val);

/* reorder_off_diag2 (hecmw_matrix_reorder.f90:98-140) for NDOF x NDOF blocks */
static void reorder_off_diag_nn(int nd, int32_t N, const int32_t *iperm, const int32_t *indexX, const int32_t *itemX,
                                const double *AX, const int32_t *indexLp, const int32_t *indexUp, const int32_t *itemLp,
                                const int32_t *itemUp, double *ALp, double *AUp) {
  const size_t nd2 = (size_t)nd * nd;
  for (int32_t iold = 1; iold <= N; iold++) {
    const int32_t inew = F1(iperm, iold);
    for (int32_t jold = indexX[iold - 1] + 1; jold <= indexX[iold]; jold++) {
      const int32_t kold = F1(itemX, jold);
      if (kold > N) continue;
      const int32_t knew = F1(iperm, kold);
      if (knew < inew) {
        const int32_t jnew = bsearch_1(itemLp, indexLp[inew - 1] + 1, indexLp[inew], knew);
        memcpy(&ALp[nd2 * (jnew - 1)], &AX[nd2 * (jold - 1)], nd2 * sizeof(double));
      } else {
        const int32_t jnew = bsearch_1(itemUp, indexUp[inew - 1] + 1, indexUp[inew], knew);
        memcpy(&AUp[nd2 * (jnew - 1)], &AX[nd2 * (jold - 1)], nd2 * sizeof(double));
      }
    }
  }
}

static void ssor_nn_setup(orc_precond *P, const orc_matrix *A, double SIGMA_DIAG, int NCOLOR_IN, int nthreads) {
  const int nd = P->ndof;
  const size_t nd2 = (size_t)nd * nd;
  const int32_t N = A->N;
  P->perm = (int32_t *)calloc((size_t)N, sizeof(int32_t));
  P->iperm = (int32_t *)calloc((size_t)N, sizeof(int32_t));
  if (nthreads == 1) { /* :91-99 */
    P->NColor = 1;
    P->COLORindex = (int32_t *)calloc(2, sizeof(int32_t));
    P->COLORindex[1] = N;
    for (int32_t i = 1; i <= N; i++) { F1(P->perm, i) = i; F1(P->iperm, i) = i; }
  } else { /* :100-109 */
    P->COLORindex = (int32_t *)calloc((size_t)N + 1, sizeof(int32_t));
    int32_t *perm_tmp = (int32_t *)calloc((size_t)N, sizeof(int32_t));
    orc_ordering_rcm(N, A->indexL, A->itemL, A->indexU, A->itemU, perm_tmp, P->iperm);
    orc_ordering_mc(N, A->indexL, A->itemL, A->indexU, A->itemU, perm_tmp, NCOLOR_IN, &P->NColor, P->COLORindex, P->perm,
                    P->iperm);
    free(perm_tmp);
  }
  const int32_t NPL = A->indexL[N], NPU = A->indexU[N];
  P->indexL = (int32_t *)calloc((size_t)N + 1, sizeof(int32_t));
  P->indexU = (int32_t *)calloc((size_t)N + 1, sizeof(int32_t));
  P->itemL = (int32_t *)calloc((size_t)NPL + NPU + 1, sizeof(int32_t));
  P->itemU = (int32_t *)calloc((size_t)NPL + NPU + 1, sizeof(int32_t));
  reorder_profile(N, P->perm, P->iperm, A->indexL, A->indexU, A->itemL, A->itemU, P->indexL, P->indexU, P->itemL, P->itemU);
  P->D = (double *)calloc(nd2 * N, sizeof(double));
  P->AL = (double *)calloc(nd2 * ((size_t)NPL + NPU) + nd2, sizeof(double));
  P->AU = (double *)calloc(nd2 * ((size_t)NPL + NPU) + nd2, sizeof(double));
  for (int32_t iold = 1; iold <= N; iold++)
    memcpy(&P->D[nd2 * (F1(P->iperm, iold) - 1)], &A->D[nd2 * (iold - 1)], nd2 * sizeof(double));
  reorder_off_diag_nn(nd, N, P->iperm, A->indexL, A->itemL, A->AL, P->indexL, P->indexU, P->itemL, P->itemU, P->AL, P->AU);
  reorder_off_diag_nn(nd, N, P->iperm, A->indexU, A->itemU, A->AU, P->indexL, P->indexU, P->itemL, P->itemU, P->AL, P->AU);
  for (int32_t i = 1; i <= P->indexL[N]; i++) F1(P->itemL, i) = F1(P->perm, F1(P->itemL, i)); /* renum_item: OLD ids */
  for (int32_t i = 1; i <= P->indexU[N]; i++) F1(P->itemU, i) = F1(P->perm, F1(P->itemU, i));
  P->ALU = (double *)calloc(nd2 * N, sizeof(double));
  memcpy(P->ALU, P->D, nd2 * N * sizeof(double));
  for (int32_t ii = 0; ii < N; ii++) lu_nn(nd, &P->ALU[nd2 * ii], SIGMA_DIAG);
}

static void ssor_nn_apply(const orc_precond *P, double *ZP) {
  const int nd = P->ndof;
  const size_t nd2 = (size_t)nd * nd;
  double SW[16], X[16];
  for (int32_t ic = 1; ic <= P->NColor; ic++) { /* FORWARD :291-336 */
    for (int32_t i = P->COLORindex[ic - 1] + 1; i <= P->COLORindex[ic]; i++) {
      const int32_t iold = F1(P->perm, i);
      for (int d = 0; d < nd; d++) SW[d] = ZP[(size_t)nd * (iold - 1) + d];
      for (int32_t j = P->indexL[i - 1] + 1; j <= P->indexL[i]; j++) {
        const int32_t k = F1(P->itemL, j);
        for (int d = 0; d < nd; d++) X[d] = ZP[(size_t)nd * (k - 1) + d];
        for (int d = 0; d < nd; d++)
          for (int e = 0; e < nd; e++) SW[d] = SW[d] - P->AL[nd2 * (j - 1) + nd * d + e] * X[e];
      }
      lusolve_nn_q(nd, &P->ALU[nd2 * (i - 1)], SW, nd == 6);
      for (int d = 0; d < nd; d++) ZP[(size_t)nd * (iold - 1) + d] = SW[d];
    }
  }
  for (int32_t ic = P->NColor; ic >= 1; ic--) { /* BACKWARD :339-406 */
    for (int32_t i = P->COLORindex[ic]; i >= P->COLORindex[ic - 1] + 1; i--) {
      for (int d = 0; d < nd; d++) SW[d] = 0.0;
      for (int32_t j = P->indexU[i]; j >= P->indexU[i - 1] + 1; j--) {
        const int32_t k = F1(P->itemU, j);
        for (int d = 0; d < nd; d++) X[d] = ZP[(size_t)nd * (k - 1) + d];
        for (int d = 0; d < nd; d++)
          for (int e = 0; e < nd; e++) SW[d] = SW[d] + P->AU[nd2 * (j - 1) + nd * d + e] * X[e];
      }
      lusolve_nn_q(nd, &P->ALU[nd2 * (i - 1)], SW, nd == 6);
      const int32_t iold = F1(P->perm, i);
      for (int d = 0; d < nd; d++) ZP[(size_t)nd * (iold - 1) + d] -= SW[d];
    }
  }
}

/* ILU1bNN (BILU_nn.f90:1539-1567 == ILU1b44 / ILU1b66): RHS = Aik * DkINV^-1 * Akj, column by column.  The unrolled copies start
 * each sum with its first product (ILU1b66 :2222), the generic one with 0.0 + it: the same value, so the unrolled form is kept. */
static void ilu1b_nn(int nd, double *RHS, const double *DkINV, const double *Aik, const double *Akj) {
  double X[16];
  for (int c = 0; c < nd; c++) {
    for (int r = 0; r < nd; r++) X[r] = Akj[r * nd + c];
    lusolve_nn(nd, DkINV, X);
    for (int r = 0; r < nd; r++) {
      double s = Aik[r * nd] * X[0];
      for (int q = 1; q < nd; q++) s = s + Aik[r * nd + q] * X[q];
      RHS[r * nd + c] = s;
    }
  }
}

/* FORM_ILU0_nn, BILU_nn.f90:196-333.  Rows 2..NP in natural order; the LU of the diagonal block of row i (ILU1aNN == lu_nn)
 * is taken in place once its updates are done.  FORM_ILU0_66 keeps Dlu0 unfactored and takes ILU1a66 of D_k again for every
 * use and of every row at the end (BILU_66.f90:65-123): the same LU of the same block, so the same bits.  As in the 3x3
 * restatement only the touched entries of IW1 / IW2 are reset.  Halo columns of U are updated like any other and later
 * multiply ZP(halo) = 0 in the apply; halo rows are factored too (nothing of rows 1..N depends on them). */
static void ilu0_nn_setup(orc_precond *P, const orc_matrix *A, double SIGMA_DIAG) {
  const int nd = P->ndof;
  const size_t nd2 = (size_t)nd * nd;
  const int32_t NP = A->NP, NPL = A->indexL[NP], NPU = A->indexU[NP];
  const int32_t *INL = A->indexL, *INU = A->indexU, *IAL = A->itemL, *IAU = A->itemU;
  P->Dlu0 = (double *)malloc(nd2 * ((size_t)NP + 1) * sizeof(double));
  P->ALlu0 = (double *)malloc(nd2 * ((size_t)NPL + 1) * sizeof(double));
  P->AUlu0 = (double *)malloc(nd2 * ((size_t)NPU + 1) * sizeof(double));
  memcpy(P->Dlu0, A->D, nd2 * NP * sizeof(double));
  memcpy(P->ALlu0, A->AL, nd2 * NPL * sizeof(double));
  memcpy(P->AUlu0, A->AU, nd2 * NPU * sizeof(double));
  P->inumFI1L = INL; P->inumFI1U = INU; P->FI1L = IAL; P->FI1U = IAU;
  double *Dlu0 = P->Dlu0, *ALlu0 = P->ALlu0, *AUlu0 = P->AUlu0;
  int32_t *IW1 = (int32_t *)calloc((size_t)NP + 1, sizeof(int32_t));
  int32_t *IW2 = (int32_t *)calloc((size_t)NP + 1, sizeof(int32_t));
  for (int32_t i = 0; i < NP; i++)
    for (int d = 0; d < nd; d++) Dlu0[nd2 * i + (size_t)(nd + 1) * d] *= SIGMA_DIAG; /* :245-249 */
  if (NP > 0) lu_nn(nd, &Dlu0[0], 1.0); /* i = 1, :251-257 */
  for (int32_t i = 2; i <= NP; i++) {
    for (int32_t k = INL[i - 1] + 1; k <= INL[i]; k++) IW1[F1(IAL, k)] = k;
    for (int32_t k = INU[i - 1] + 1; k <= INU[i]; k++) IW2[F1(IAU, k)] = k;
    for (int32_t kk = INL[i - 1] + 1; kk <= INL[i]; kk++) {
      const int32_t k = F1(IAL, kk);
      const double *DkINV = &Dlu0[nd2 * (k - 1)];
      double Aik[36], RHS[36];
      memcpy(Aik, &ALlu0[nd2 * (kk - 1)], nd2 * sizeof(double));
      for (int32_t jj = INU[k - 1] + 1; jj <= INU[k]; jj++) {
        const int32_t j = F1(IAU, jj);
        if (IW1[j] == 0 && IW2[j] == 0) continue; /* j == i is never listed: the diagonal update below is dead, as in the 3x3 */
        ilu1b_nn(nd, RHS, DkINV, Aik, &AUlu0[nd2 * (jj - 1)]);
        double *dst = j == i ? &Dlu0[nd2 * (i - 1)] : j < i ? &ALlu0[nd2 * (IW1[j] - 1)] : &AUlu0[nd2 * (IW2[j] - 1)];
        for (size_t q = 0; q < nd2; q++) dst[q] = dst[q] - RHS[q];
      }
    }
    lu_nn(nd, &Dlu0[nd2 * (i - 1)], 1.0);
    for (int32_t k = INL[i - 1] + 1; k <= INL[i]; k++) IW1[F1(IAL, k)] = 0;
    for (int32_t k = INU[i - 1] + 1; k <= INU[i]; k++) IW2[F1(IAU, k)] = 0;
  }
  free(IW1); free(IW2);
}

/* hecmw_precond_BILU_nn_apply, BILU_nn.f90:90-168 (== BILU_44 / _66 apply): rows 1..N, forward ascending with L in stored
 * order, backward descending with U in reverse stored order */
static void ilu_nn_apply(const orc_precond *P, double *WW) {
  const int nd = P->ndof;
  const size_t nd2 = (size_t)nd * nd;
  double SW[16], X[16];
  for (int32_t i = 1; i <= P->N; i++) {
    for (int d = 0; d < nd; d++) SW[d] = WW[(size_t)nd * (i - 1) + d];
    for (int32_t j = P->inumFI1L[i - 1] + 1; j <= P->inumFI1L[i]; j++) {
      const int32_t k = F1(P->FI1L, j);
      for (int d = 0; d < nd; d++) X[d] = WW[(size_t)nd * (k - 1) + d];
      for (int d = 0; d < nd; d++)
        for (int e = 0; e < nd; e++) SW[d] = SW[d] - P->ALlu0[nd2 * (j - 1) + nd * d + e] * X[e];
    }
    lusolve_nn(nd, &P->Dlu0[nd2 * (i - 1)], SW);
    for (int d = 0; d < nd; d++) WW[(size_t)nd * (i - 1) + d] = SW[d];
  }
  for (int32_t i = P->N; i >= 1; i--) {
    for (int d = 0; d < nd; d++) SW[d] = 0.0;
    for (int32_t j = P->inumFI1U[i]; j >= P->inumFI1U[i - 1] + 1; j--) {
      const int32_t k = F1(P->FI1U, j);
      for (int d = 0; d < nd; d++) X[d] = WW[(size_t)nd * (k - 1) + d];
      for (int d = 0; d < nd; d++)
        for (int e = 0; e < nd; e++) SW[d] = SW[d] + P->AUlu0[nd2 * (j - 1) + nd * d + e] * X[e];
    }
    lusolve_nn(nd, &P->Dlu0[nd2 * (i - 1)], SW);
    for (int d = 0; d < nd; d++) WW[(size_t)nd * (i - 1) + d] -= SW[d];
  }
}
