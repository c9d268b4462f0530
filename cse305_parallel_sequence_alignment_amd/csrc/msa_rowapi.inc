// msa_rowapi.inc -- C-ABI over rowsweep_kernel (msa_rowsweep.hip): the
// reference's double-precision tables for any g, h, and its per-row / per-range
// steps for the source-compatible `class Subproblem` (subproblem_alignment.h).
// Included by msa_capi.hip after msa_devcall.inc (uses DeviceCall; neither entry reserves a footprint).

extern "C" {

int msa_subproblem_f64(const char* A1, const char* B1, size_t m_in, size_t n_in, size_t idA_in, size_t idB_in,
                       int start_type, double g, double h, int mode, double* T1, double* T2, double* T3,
                       int* invert) {
  if (!A1 || !B1 || !T1 || !T2 || !T3 || (m_in == 0 && n_in == 0)) return MSA_ERR_ARG;
  if (mode != MSA_F64_COMPUTE_TABLES && mode != MSA_F64_NON_PARALLEL) return MSA_ERR_ARG;
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  // constructor swap (subproblem_alignment.h:37-54)
  const bool inv = m_in > n_in;
  const char* A = inv ? B1 : A1;
  const char* B = inv ? A1 : B1;
  const size_t m = inv ? n_in : m_in, n = inv ? m_in : n_in;
  const size_t idA = inv ? idB_in : idA_in, idB = inv ? idA_in : idB_in;
  if (invert) *invert = inv ? 1 : 0;
  const size_t W = n + 1, cells = (m + 1) * W;
  DeviceCall dc(0);
  if ((rc = dc.status()) != MSA_OK) return rc;
  void *dA, *dB, *dv, *dT[3];
  if (!(dA = dc.alloc(m + 1)) || !(dB = dc.alloc(n + 1)) || !(dv = dc.alloc(sizeof(double) * W))) return MSA_ERR_NOMEM;
  for (auto& t : dT)
    if (!(t = dc.alloc(sizeof(double) * cells))) return MSA_ERR_NOMEM;
  // A[k] = reference A[id_A + k], B[j] = reference B[id_B + j] (f, subproblem_alignment.h:83-88)
  if ((rc = dc.upload(dA, A + idA, m + 1)) || (rc = dc.upload(dB, B + idB, n + 1))) return rc;
  RowArgs a;
  std::memset(&a, 0, sizeof(a));
  a.T1 = (double*)dT[0];
  a.T2 = (double*)dT[1];
  a.T3 = (double*)dT[2];
  a.W = (long long)W;
  a.n = (long long)n;
  a.A = (const char*)dA;
  a.B = (const char*)dB;
  a.g = g;
  a.h = h;
  a.start_type = start_type;
  a.vec = (double*)dv;
  a.part = ROW_ZERO;  // compute_tables (:329-332): row 0, then rows 1..m in order
  a.i0 = 0;
  a.i1 = 1;
  a.slot0 = 0;
  hipLaunchKernelGGL(rowsweep_kernel, dim3(1), dim3(RS_THREADS), 0, dc.stream(), a);
  HIPCHK(hipGetLastError());
  if (m > 0) {
    a.part = ROW_FULL | (mode == MSA_F64_NON_PARALLEL ? ROW_SEQ : 0);
    a.i0 = 1;
    a.i1 = (long long)m + 1;
    a.slot0 = 1;
    hipLaunchKernelGGL(rowsweep_kernel, dim3(1), dim3(RS_THREADS), 0, dc.stream(), a);
    HIPCHK(hipGetLastError());
  }
  double* outs[3] = {T1, T2, T3};
  for (int v = 0; v < 3; ++v)
    if ((rc = dc.download(outs[v], dT[v], sizeof(double) * cells))) return rc;
  return dc.sync();
}

int msa_subproblem_row(int part, const char* A1, const char* B1, size_t idA, size_t idB, size_t n, size_t i,
                       int start_type, double g, double h, size_t start, size_t end, const double* up1,
                       const double* up2, const double* up3, double* cur1, double* cur2, double* cur3, double* vec) {
  if (!A1 || !B1 || !cur1 || !cur2 || !cur3) return MSA_ERR_ARG;
  const bool needs_up = part == MSA_ROW_13 || part == MSA_ROW_FULL;
  if (part != MSA_ROW_FIRST && part != MSA_ROW_13 && part != MSA_ROW_OMEGA && part != MSA_ROW_T2 &&
      part != MSA_ROW_ZERO && part != MSA_ROW_FULL)
    return MSA_ERR_ARG;
  if (needs_up && (i == 0 || !up1 || !up2 || !up3)) return MSA_ERR_ARG;
  if ((part == MSA_ROW_OMEGA || part == MSA_ROW_T2) && !vec) return MSA_ERR_ARG;
  // the MapThread ranges index j-1 (13, omega): columns start at 1
  if (part != MSA_ROW_ZERO && part != MSA_ROW_FULL && (start > end || end > n + 1 || start < 1)) return MSA_ERR_ARG;
  int rc = ensure_device();
  if (rc != MSA_OK) return rc;
  const size_t W = n + 1;
  DeviceCall dc(0);
  if ((rc = dc.status()) != MSA_OK) return rc;
  void *dA, *dB, *dv, *dT[3];
  if (!(dA = dc.alloc(1)) || !(dB = dc.alloc(W)) || !(dv = dc.alloc(sizeof(double) * W))) return MSA_ERR_NOMEM;
  for (auto& t : dT)
    if (!(t = dc.alloc(sizeof(double) * 2 * W))) return MSA_ERR_NOMEM;  // slot 0 = row i-1, slot 1 = row i
  if ((rc = dc.upload(dA, A1 + idA + i, 1)) || (rc = dc.upload(dB, B1 + idB, W))) return rc;
  const double* ups[3] = {up1, up2, up3};
  double* curs[3] = {cur1, cur2, cur3};
  for (int v = 0; v < 3; ++v) {
    if (needs_up && (rc = dc.upload(dT[v], ups[v], sizeof(double) * W))) return rc;
    if ((rc = dc.upload((double*)dT[v] + W, curs[v], sizeof(double) * W))) return rc;
  }
  if (vec && (rc = dc.upload(dv, vec, sizeof(double) * W))) return rc;
  RowArgs a;
  std::memset(&a, 0, sizeof(a));
  a.T1 = (double*)dT[0];
  a.T2 = (double*)dT[1];
  a.T3 = (double*)dT[2];
  a.W = (long long)W;
  a.n = (long long)n;
  a.i0 = (long long)i;
  a.i1 = (long long)i + 1;
  a.slot0 = 1;
  a.A = (const char*)dA - (long long)i;  // only A[i] is read
  a.B = (const char*)dB;
  a.g = g;
  a.h = h;
  a.start_type = start_type;
  a.part = part;
  a.start = (long long)start;
  a.end = (long long)end;
  a.vec = (double*)dv;
  hipLaunchKernelGGL(rowsweep_kernel, dim3(1), dim3(RS_THREADS), 0, dc.stream(), a);
  HIPCHK(hipGetLastError());
  // copy back only what the part wrote: the reference runs MapThread bodies on
  // disjoint column ranges of one row from several threads at once (:294-325)
  const bool whole = part == MSA_ROW_ZERO || part == MSA_ROW_FULL;
  const size_t c0 = whole ? 0 : start, c1 = whole ? W : end;
  const bool wrote[3] = {part != MSA_ROW_OMEGA && part != MSA_ROW_T2,
                         part != MSA_ROW_OMEGA && part != MSA_ROW_13,
                         part != MSA_ROW_OMEGA && part != MSA_ROW_T2};
  for (int v = 0; v < 3; ++v)
    if (wrote[v] && c1 > c0 &&
        (rc = dc.download(curs[v] + c0, (double*)dT[v] + W + c0, sizeof(double) * (c1 - c0))))
      return rc;
  if (part == MSA_ROW_OMEGA && c1 > c0 && (rc = dc.download(vec + c0, (double*)dv + c0, sizeof(double) * (c1 - c0))))
    return rc;
  return dc.sync();
}

}  // extern "C"
