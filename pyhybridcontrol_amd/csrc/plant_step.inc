// The arithmetic of one plant step -- the reference's MldModel.lsim_k (models/mld_model.py:690-694) -- once, for k_advance (kernels.inc), k_sim_step
// (sim_step.inc) and ro_run (rollout.inc):
//     x_k1 = b5 + A x + [B1 B2 B3 0] v + B4 omega ,  y = d5 + C x + [D1 D2 D3 0] v + D4 omega                      plant_row
//     r    = E x + [F1 F2 F3] (u, delta, z) + F4 omega + G y - f5                                                   plant_residual
//     cons_vio = max_i r_i, cons_row = the lowest row that attains it; a NaN residual wins                         plant_worst, plant_worst_merge
// The order of every sum is fixed HERE (start from the affine term, then x, v, omega [, y], j ascending, s += a * b): the three callers agree bit for bit
// because they call these functions (tests/test_gpu_sim_step.py::test_same_bits_as_advance, tests/test_gpu_rollout.py::test_plant_rows_equal_sim_step_bit_for_bit).
// Compiles for the device and, with SM_HOST defined (small_lds.inc), for a host program without the HIP runtime.  The operand vectors are templated on
// their pointer type: k_sim_step reads generic pointers (LDS or global memory), ro_run the wave's LDS staging (sm_f64 *).
#pragma once
#include <stddef.h>
#ifdef SM_HOST
#define PLANT_FN static inline
#else
#define PLANT_FN __device__ __forceinline__
#endif

// offsets (in doubles) of the matrices inside one model's block of mld_model::d_pack; Bv = [B1 B2 B3 0], Dv = [D1 D2 D3 0], Fv = [F1 F2 F3 Psi], each nv wide
struct PackOff { size_t A, B4, b5, C, D4, d5, E, F4, f5, G, Bv, Dv, Fv; };
// the same matrices by pointer: one model's block resolved (ro_run keeps the thirteen over the K steps of a trajectory)
struct PlantMats { const double *A, *B4, *b5, *C, *D4, *d5, *E, *F4, *f5, *G, *Bv, *Dv, *Fv; };
PLANT_FN PlantMats plant_mats(const double *pk, const PackOff &o)
{
    return PlantMats{pk + o.A, pk + o.B4, pk + o.b5, pk + o.C, pk + o.D4, pk + o.d5, pk + o.E, pk + o.F4, pk + o.f5, pk + o.G, pk + o.Bv, pk + o.Dv, pk + o.Fv};
}

// row i of  b + M x + Mv v + M4 omega  (M: rows x nx, Mv: rows x nv, M4: rows x nw, row-major): the state rows with (b5, A, Bv, B4), the output rows with (d5, C, Dv, D4)
template <typename X, typename V, typename W>
PLANT_FN double plant_row(int i, const double *b, const double *M, const double *Mv, const double *M4, int nx, int nv, int nw, X x, V v, W w)
{
    double s = b[i];
    for (int j = 0; j < nx; ++j) s += M[(size_t)i * nx + j] * x[j];
    for (int j = 0; j < nv; ++j) s += Mv[(size_t)i * nv + j] * v[j];
    for (int j = 0; j < nw; ++j) s += M4[(size_t)i * nw + j] * w[j];
    return s;
}

// residual of constraint row i; nf = nv - nmu: the Psi columns, the last nmu of a row of Fv, are skipped
template <typename X, typename V, typename W, typename Y>
PLANT_FN double plant_residual(int i, const double *E, const double *Fv, const double *F4, const double *G, const double *f5, int nx, int nv, int nf, int nw, int ny,
                               X x, V v, W w, Y y)
{
    double s = 0.0;
    for (int j = 0; j < nx; ++j) s += E[(size_t)i * nx + j] * x[j];
    for (int j = 0; j < nf; ++j) s += Fv[(size_t)i * nv + j] * v[j];
    for (int j = 0; j < nw; ++j) s += F4[(size_t)i * nw + j] * w[j];
    for (int j = 0; j < ny; ++j) s += G[(size_t)i * ny + j] * y[j];
    return s - f5[i];
}

// a lane's running (largest residual, its row), fed rows in ascending order; starts as (anything, -1).  The first of equals stays, a NaN beats any number
PLANT_FN void plant_worst(double s, int i, double &best, int &brow)
{
    const bool s_nan = s != s, b_nan = best != best;
    if (brow < 0 || (!b_nan && (s_nan || s > best))) { best = s; brow = i; }
}

// another lane's (ob, orow) merged into this lane's: a NaN wins, ties go to the lower row, a lane without rows (orow < 0) never wins
PLANT_FN void plant_worst_merge(double ob, int orow, double &best, int &brow)
{
    const bool o_nan = ob != ob, m_nan = best != best;
    bool take;
    if (orow < 0) take = false;
    else if (brow < 0) take = true;
    else if (o_nan || m_nan) take = o_nan && (!m_nan || orow < brow);
    else take = ob > best || (ob == best && orow < brow);
    if (take) { best = ob; brow = orow; }
}
