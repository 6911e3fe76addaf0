// Pose graph (include/loamx.h, loamx_posegraph_*): the FP64 definitions shared by the host-only entry points and the kernels of
// posegraph.hip.  Every function below is plain C++ with one fixed order of operations (the library is built with -ffp-contract=off),
// so the host and the device evaluate the same expressions; only sin, cos, atan2 and sqrt come from different libraries.
//
// A pose is double[12], row-major 3x4 (R | t).  A 3x3 matrix is double[9], row-major.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PG_HD __host__ __device__ inline
#else
#define PG_HD inline
#endif

namespace loamx {

constexpr double PG_SMALL_ANGLE = 1e-8;   // below it Exp, Log and Jr^-1 take their series branch (part of the definition)

PG_HD void pg_rot(const double* T, double* R) {
  R[0] = T[0]; R[1] = T[1]; R[2] = T[2];
  R[3] = T[4]; R[4] = T[5]; R[5] = T[6];
  R[6] = T[8]; R[7] = T[9]; R[8] = T[10];
}
// C = A B;  C = A^T B;  C = A B^T  (each entry: three products added left to right)
PG_HD void pg_mm(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
PG_HD void pg_mtm(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
PG_HD void pg_mmt(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}
PG_HD void pg_mv(const double* A, const double* v, double* o) {
  for (int i = 0; i < 3; i++) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
PG_HD void pg_mtv(const double* A, const double* v, double* o) {
  for (int i = 0; i < 3; i++) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
PG_HD void pg_hat(const double* w, double* K) {
  K[0] = 0.0; K[1] = -w[2]; K[2] = w[1];
  K[3] = w[2]; K[4] = 0.0; K[5] = -w[0];
  K[6] = -w[1]; K[7] = w[0]; K[8] = 0.0;
}

// Exp(w) = I + a [w]x + b [w]x^2;  a = sin|w| / |w|, b = (1 - cos|w|) / |w|^2;  below PG_SMALL_ANGLE: a = 1, b = 1/2
PG_HD void pg_exp(const double* w, double* R) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double th = sqrt(th2);
  double a = 1.0, b = 0.5;
  if (th >= PG_SMALL_ANGLE) {
    a = sin(th) / th;
    b = (1.0 - cos(th)) / th2;
  }
  double K[9], K2[9];
  pg_hat(w, K);
  pg_mm(K, K, K2);
  for (int i = 0; i < 9; i++) R[i] = a * K[i] + b * K2[i];
  R[0] = 1.0 + R[0];
  R[4] = 1.0 + R[4];
  R[8] = 1.0 + R[8];
}

// Log(R): v = the vector of (R - R^T) / 2 (= sin(angle) * axis), c = (trace - 1) / 2, angle = atan2(|v|, c) in [0, pi];
// phi = v * angle / |v|;  below PG_SMALL_ANGLE: phi = v
PG_HD void pg_log(const double* R, double* phi) {
  const double v0 = 0.5 * (R[7] - R[5]), v1 = 0.5 * (R[2] - R[6]), v2 = 0.5 * (R[3] - R[1]);
  const double c = 0.5 * ((R[0] + R[4] + R[8]) - 1.0);
  const double s = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  const double th = atan2(s, c);
  double k = 1.0;
  if (th >= PG_SMALL_ANGLE) k = th / s;
  phi[0] = k * v0;
  phi[1] = k * v1;
  phi[2] = k * v2;
}

// Q = Jr^-1(phi) = I + 1/2 [phi]x + q [phi]x^2;  q = 1/|phi|^2 - (1 + cos|phi|) / (2 |phi| sin|phi|);  below PG_SMALL_ANGLE: q = 1/12
PG_HD void pg_jrinv(const double* phi, double* Q) {
  const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  const double th = sqrt(th2);
  double q = 1.0 / 12.0;
  if (th >= PG_SMALL_ANGLE) q = 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
  double K[9], K2[9];
  pg_hat(phi, K);
  pg_mm(K, K, K2);
  for (int i = 0; i < 9; i++) Q[i] = 0.5 * K[i] + q * K2[i];
  Q[0] = 1.0 + Q[0];
  Q[4] = 1.0 + Q[4];
  Q[8] = 1.0 + Q[8];
}

// the intermediate quantities of one edge's residual, kept for the Jacobians
struct PgResidual {
  double RA[9], tA[3], RE[9], r[6];
};
PG_HD void pg_residual(const double* Ti, const double* Tj, const double* Z, PgResidual& o) {
  double Ri[9], Rj[9], Rz[9];
  pg_rot(Ti, Ri);
  pg_rot(Tj, Rj);
  pg_rot(Z, Rz);
  const double d[3] = {Tj[3] - Ti[3], Tj[7] - Ti[7], Tj[11] - Ti[11]};
  pg_mtm(Ri, Rj, o.RA);
  pg_mtv(Ri, d, o.tA);
  pg_mtm(Rz, o.RA, o.RE);
  const double e[3] = {o.tA[0] - Z[3], o.tA[1] - Z[7], o.tA[2] - Z[11]};
  pg_mtv(Rz, e, o.r);
  pg_log(o.RE, o.r + 3);
}

// z = Ti^-1 Tj
PG_HD void pg_between(const double* Ti, const double* Tj, double* z) {
  double Ri[9], Rj[9], RA[9], tA[3];
  pg_rot(Ti, Ri);
  pg_rot(Tj, Rj);
  const double d[3] = {Tj[3] - Ti[3], Tj[7] - Ti[7], Tj[11] - Ti[11]};
  pg_mtm(Ri, Rj, RA);
  pg_mtv(Ri, d, tA);
  for (int i = 0; i < 3; i++) {
    z[4 * i] = RA[3 * i]; z[4 * i + 1] = RA[3 * i + 1]; z[4 * i + 2] = RA[3 * i + 2];
    z[4 * i + 3] = tA[i];
  }
}

// index of entry (k, m) of a symmetric 6x6 matrix in its 21 upper-triangle entries, row-major
PG_HD int pg_tri(int k, int m) {
  const int a = k < m ? k : m, b = k < m ? m : k;
  return a * 6 - a * (a - 1) / 2 + (b - a);
}
PG_HD double pg_chi2(const double* info, const double* r) {
  double acc = 0.0;
  for (int k = 0; k < 6; k++) {
    double row = 0.0;
    for (int m = 0; m < 6; m++) row = row + info[pg_tri(k, m)] * r[m];
    acc = acc + r[k] * row;
  }
  return acc;
}
// IRLS weight and rho of one edge (robust: the edge is flagged and huber_delta > 0)
PG_HD void pg_huber(double chi2, bool robust, double delta, double& w, double& rho) {
  w = 1.0;
  rho = chi2;
  if (robust && chi2 > delta * delta) {
    const double s = sqrt(chi2);
    w = delta / s;
    rho = 2.0 * delta * s - delta * delta;
  }
}

// The Jacobians of r at delta = 0 as one dense 6x12 matrix J = (J_i | J_j), row-major (rows t, phi; columns v_i, w_i, v_j, w_j):
//   J_j = [[R_E, 0], [0, Q]],  J_i = [[-R_z^T, R_z^T [t_A]x], [0, -Q R_A^T]],  Q = Jr^-1(phi)
PG_HD void pg_jacobians(const double* Z, const PgResidual& s, double* J) {
  double Rz[9], Q[9], K[9], B[9], Cm[9];
  pg_rot(Z, Rz);
  pg_jrinv(s.r + 3, Q);
  pg_hat(s.tA, K);
  pg_mtm(Rz, K, B);
  pg_mmt(Q, s.RA, Cm);
  for (int i = 0; i < 72; i++) J[i] = 0.0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      J[12 * a + b] = -Rz[3 * b + a];
      J[12 * a + 3 + b] = B[3 * a + b];
      J[12 * (3 + a) + 3 + b] = -Cm[3 * a + b];
      J[12 * a + 6 + b] = s.RE[3 * a + b];
      J[12 * (3 + a) + 9 + b] = Q[3 * a + b];
    }
}

// Retraction of one pose by delta = (v, w): t <- t + R v, R <- R Exp(w), then R is made orthonormal again by Gram-Schmidt on its
// columns: c0 normalised, c1 minus its part along c0 and normalised, c2 = c0 x c1.
PG_HD void pg_retract(double* T, const double* delta) {
  double R[9], E[9], N[9], Rv[3];
  pg_rot(T, R);
  pg_mv(R, delta, Rv);
  pg_exp(delta + 3, E);
  pg_mm(R, E, N);
  double c0[3] = {N[0], N[3], N[6]}, c1[3] = {N[1], N[4], N[7]};
  const double n0 = sqrt(c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2]);
  for (int i = 0; i < 3; i++) c0[i] = c0[i] / n0;
  const double d = c0[0] * c1[0] + c0[1] * c1[1] + c0[2] * c1[2];
  for (int i = 0; i < 3; i++) c1[i] = c1[i] - d * c0[i];
  const double n1 = sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
  for (int i = 0; i < 3; i++) c1[i] = c1[i] / n1;
  const double c2[3] = {c0[1] * c1[2] - c0[2] * c1[1], c0[2] * c1[0] - c0[0] * c1[2], c0[0] * c1[1] - c0[1] * c1[0]};
  for (int i = 0; i < 3; i++) {
    T[4 * i] = c0[i];
    T[4 * i + 1] = c1[i];
    T[4 * i + 2] = c2[i];
    T[4 * i + 3] = T[4 * i + 3] + Rv[i];
  }
}

}  // namespace loamx
