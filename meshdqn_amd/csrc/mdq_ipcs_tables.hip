// IPCS, shared: the reference-element tables on the host (build_tables) and their upload into the including unit's c_tab
// (upload_tables).  Included by all four IPCS units, behind its kernels.
namespace mdq {

// ================================================================== host side

static void build_tables(RefTab& T) {
  const double s15 = std::sqrt(15.0);
  const double a1 = (6.0 - s15) / 21.0, a2 = (6.0 + s15) / 21.0;
  const double w0 = 9.0 / 40.0, w1 = (155.0 - s15) / 1200.0, w2 = (155.0 + s15) / 1200.0;
  const double pts[NQ][2] = {{1.0 / 3.0, 1.0 / 3.0}, {a1, a1}, {1.0 - 2.0 * a1, a1}, {a1, 1.0 - 2.0 * a1},
                             {a2, a2},               {1.0 - 2.0 * a2, a2}, {a2, 1.0 - 2.0 * a2}};
  const double wts[NQ] = {w0, w1, w1, w1, w2, w2, w2};
  auto basis = [](double xi, double eta, double* phi, double (*dphi)[2], double* psi) {
    const double lam[3] = {1.0 - xi - eta, xi, eta};
    const double dl[3][2] = {{-1.0, -1.0}, {1.0, 0.0}, {0.0, 1.0}};
    const int EA[3] = {1, 0, 0}, EB[3] = {2, 2, 1};
    for (int k = 0; k < 3; ++k) {
      psi[k] = lam[k];
      phi[k] = lam[k] * (2.0 * lam[k] - 1.0);
      dphi[k][0] = (4.0 * lam[k] - 1.0) * dl[k][0];
      dphi[k][1] = (4.0 * lam[k] - 1.0) * dl[k][1];
      phi[3 + k] = 4.0 * lam[EA[k]] * lam[EB[k]];
      dphi[3 + k][0] = 4.0 * (lam[EA[k]] * dl[EB[k]][0] + lam[EB[k]] * dl[EA[k]][0]);
      dphi[3 + k][1] = 4.0 * (lam[EA[k]] * dl[EB[k]][1] + lam[EB[k]] * dl[EA[k]][1]);
    }
  };
  std::memset(&T, 0, sizeof(T));
  for (int q = 0; q < NQ; ++q) {
    T.qw[q] = 0.5 * wts[q];
    basis(pts[q][0], pts[q][1], T.qphi[q], T.qdphi[q], T.qpsi[q]);
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) {
        T.Mhat[i][j] += T.qw[q] * T.qphi[q][i] * T.qphi[q][j];
        for (int c = 0; c < 2; ++c)
          for (int dd = 0; dd < 2; ++dd) T.Ghat[c][dd][i][j] += T.qw[q] * T.qdphi[q][i][c] * T.qdphi[q][j][dd];
      }
  }
  const double g = 0.5 / std::sqrt(3.0);
  T.gx[0] = 0.5 - g;
  T.gx[1] = 0.5 + g;
  T.gw[0] = T.gw[1] = 0.5;
}

// the reference-element tables of THIS translation unit's kernels (c_tab has internal linkage)
static hipError_t upload_tables() {
  static std::once_flag once;
  static hipError_t err = hipSuccess;
  std::call_once(once, [] {
    RefTab T;
    build_tables(T);
    err = hipMemcpyToSymbol(HIP_SYMBOL(c_tab), &T, sizeof(T));
  });
  return err;
}

}  // namespace mdq
