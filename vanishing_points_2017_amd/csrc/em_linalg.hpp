// em_linalg.hpp -- 3 x 3 linear algebra of the M-step, merge and split: the Jacobi eigen-solver, the smallest right singular vector of
// a weighted line matrix by a group of lanes, and LAPACK's answer for a single row.
// One part of em_device.hpp (the conventions, and why the unit is compiled with -ffp-contract=off, are there).
#ifndef VPK_EM_LINALG_HPP_
#define VPK_EM_LINALG_HPP_

#include "em_ctx.hpp"

namespace vpk {

// symmetric 3x3 eigen-solver (cyclic Jacobi): A = J diag(ev) J^T, J orthogonal (columns = eigenvectors)
VPK_DEV void eig3_full(double a00, double a01, double a02, double a11, double a12, double a22,
                       double ev[3], double J[3][3]) {
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) J[i][k] = (i == k) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; ++sweep) {
        double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (!(off > 0)) break;
        for (int p = 0; p < 2; ++p) {
            for (int q = p + 1; q < 3; ++q) {
                double apq = A[p][q];
                if (apq == 0) continue;
                double g = 100.0 * fabs(apq);
                if (fabs(A[p][p]) + g == fabs(A[p][p]) && fabs(A[q][q]) + g == fabs(A[q][q])) {
                    A[p][q] = 0; A[q][p] = 0;                 // negligible against both diagonals
                    continue;
                }
                double theta = (A[q][q] - A[p][p]) / (2 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                if (!(fabs(theta) < 1e150)) t = 0.5 / theta;  // avoid overflow of theta^2
                double cth = 1 / sqrt(t * t + 1);
                double sth = t * cth;
                double app = A[p][p], aqq = A[q][q];
                A[p][p] = app - t * apq;
                A[q][q] = aqq + t * apq;
                A[p][q] = 0;
                A[q][p] = 0;
                int r = 3 - p - q;
                double arp = A[r][p], arq = A[r][q];
                A[r][p] = A[p][r] = cth * arp - sth * arq;
                A[r][q] = A[q][r] = sth * arp + cth * arq;
                for (int k = 0; k < 3; ++k) {
                    double vkp = J[k][p], vkq = J[k][q];
                    J[k][p] = cth * vkp - sth * vkq;
                    J[k][q] = sth * vkp + cth * vkq;
                }
            }
        }
    }
    ev[0] = A[0][0]; ev[1] = A[1][1]; ev[2] = A[2][2];
}

// Smallest right singular vector of the row-weighted line matrix diag(r) * L (N x 3), cooperatively
// by one aligned group of G lanes (G = WAVE: the whole wave) -- stands in for V[:,2] of
// numpy.linalg.svd (vp_localisation.py:466,595).  All lanes of the group must call it together.
// rw(n) returns the row weight r_n (0 = row not selected).  Pass 0 diagonalises the 3x3 scatter
// sum r^2 l l^T (normal equations: error ~ eps * cond^2 in the small direction); every further pass
// re-accumulates the scatter IN THE ROTATED BASIS V^T l, where the entries that couple to the small
// direction are sums of small numbers (no cancellation against the large ones), and applies the
// Jacobi correction -- an implicit one-sided Jacobi SVD, accurate like LAPACK's after 2-3 passes.
template <int G, int LB = 4, class RowWeight>
VPK_DEV void group_null_vector(cgdp l, int N, RowWeight rw, double out[3]) {
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    double ev[3] = {0, 0, 0};
    for (int pass = 0; pass < 5; ++pass) {
        double g00 = 0, g01 = 0, g02 = 0, g11 = 0, g12 = 0, g22 = 0;
        // LB = four lines per step with all their loads issued first: with 16 lanes per VP a lane walks N/16
        // lines, and one L2 round trip per line was most of the M-step.  (Round 6 measured LB = 8 -- same chains, same
        // bits -- SLOWER: M-step 57.9 -> 60.3 ms of workgroup time per YUD batch; the walk is bound by its divisions
        // and the eigen-solve, not by loads in flight.)
        for (int n0 = lane() % G; n0 < N; n0 += LB * G) {
            double r[LB], a0[LB], a1[LB], a2[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                const int n = n0 + u * G;
                const bool in = n < N;
                r[u] = in ? rw(n) : 0.0;
                cgdp ln = l + 3 * (size_t)(in ? n : 0);
                a0[u] = ln[0]; a1[u] = ln[1]; a2[u] = ln[2];
            }
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                if (r[u] == 0) continue;
                double y0, y1, y2;
                if (pass == 0) {
                    y0 = r[u] * a0[u]; y1 = r[u] * a1[u]; y2 = r[u] * a2[u];
                } else {
                    y0 = r[u] * (a0[u] * V[0][0] + a1[u] * V[1][0] + a2[u] * V[2][0]);
                    y1 = r[u] * (a0[u] * V[0][1] + a1[u] * V[1][1] + a2[u] * V[2][1]);
                    y2 = r[u] * (a0[u] * V[0][2] + a1[u] * V[1][2] + a2[u] * V[2][2]);
                }
                g00 += y0 * y0; g01 += y0 * y1; g02 += y0 * y2;
                g11 += y1 * y1; g12 += y1 * y2; g22 += y2 * y2;
            }
        }
        g00 = group_sum<G>(g00); g01 = group_sum<G>(g01); g02 = group_sum<G>(g02);
        g11 = group_sum<G>(g11); g12 = group_sum<G>(g12); g22 = group_sum<G>(g22);
        const double tol = 4e-16;
        const bool conv = pass > 0 && fabs(g01) <= tol * sqrt(g00 * g11) && fabs(g02) <= tol * sqrt(g00 * g22) &&
                          fabs(g12) <= tol * sqrt(g11 * g22);
        double J[3][3];
        eig3_full(g00, g01, g02, g11, g12, g22, ev, J);
        double Vn[3][3];
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) Vn[i][k] = V[i][0] * J[0][k] + V[i][1] * J[1][k] + V[i][2] * J[2][k];
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) V[i][k] = Vn[i][k];
        if (conv) break;
        if (pass == 0) {
            // normal-equations error of the bottom eigenvector ~ eps * ev_max / (ev_mid - ev_min):
            // below 1e-13 when the two larger eigenvalues are within 1e3 -> no refinement needed
            double lo = ev[0] < ev[1] ? ev[0] : ev[1]; lo = lo < ev[2] ? lo : ev[2];
            double hi = ev[0] > ev[1] ? ev[0] : ev[1]; hi = hi > ev[2] ? hi : ev[2];
            double mid = ev[0] + ev[1] + ev[2] - lo - hi;
            if (mid - lo > 1e-3 * hi) break;
        }
    }
    int b = 0;
    if (ev[1] < ev[b]) b = 1;
    if (ev[2] < ev[b]) b = 2;
    double x = V[0][b], y = V[1][b], z = V[2][b];
    double nrm = norm3(x, y, z);                              // vp /= np.linalg.norm(vp) (:472)
    out[0] = x / nrm; out[1] = y / nrm; out[2] = z / nrm;
}

template <class RowWeight>
VPK_DEV void wave_null_vector(cgdp l, int N, RowWeight rw, double out[3]) {
    group_null_vector<WAVE>(l, N, rw, out);
}

// Third right singular vector of a 1 x 3 matrix [a b c] as LAPACK returns it (numpy.linalg.svd with
// full_matrices on one row: dgesdd -> dgelqf -> one Householder reflector H = I - tau v v^T with
// beta = -sign(a)|x|, tau = (beta - a)/beta, v = (1, b/(a-beta), c/(a-beta)); V^T = H up to the sign
// of its first row).  The reference reaches this in the hard-assignment M-step when a VP wins a
// single line (vp_localisation.py:353-369) and its `err > 1.5` test (:387) depends on this vector.
VPK_DEV void lapack_null_1row(double a, double b, double c, double out[3]) {
    double nrm = sqrt(a * a + b * b + c * c);
    double beta = a >= 0 ? -nrm : nrm;
    if (a == 0 && 1.0 / a < 0) beta = nrm;                   // sign(-0.0)
    double tau = (beta - a) / beta;
    double v1 = b / (a - beta), v2 = c / (a - beta);
    out[0] = -tau * v2;
    out[1] = -tau * v2 * v1;
    out[2] = 1 - tau * v2 * v2;
}

}  // namespace vpk
#endif
