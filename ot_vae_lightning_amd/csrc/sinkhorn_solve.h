// The solver of sinkhorn.hip for the other translation units of the library (sinkhorn_div.hip): nb problems C[nb][N][M] with uniform
// marginals, each solved on C / max(pmax[b][0 .. P - 1]) for exactly max_iter iterations -- sinkhorn_impl as otvae_sinkhorn_prior_fwd
// calls it, hence the same route (sk_route) and the same bits.  ws: otvae_sinkhorn_ws(dtype, nb, N, M) bytes.  Not part of the C ABI.
#pragma once
#include "common.h"

int otvae_sk_solve_uniform(int dtype, const void* C, int nb, int N, int M, double reg, int max_iter, const void* pmax, int P, void* ws,
                           void* pi, void* u, void* v, int32_t* iters_done, hipStream_t st);
