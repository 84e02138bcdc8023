/* The cut arithmetic of csrc/mesh_cuts.h as a flat list of ints (tests/test_mesh_cuts.py compiles this with the host compiler).
 * out, per slab: nl | per level l < nl: k0 k1 lo hi | per link l + 1 < nl: the 21 ints of aa_mesh_create_local, corr_to[2] |
 * ncorr_in | per entry: level side src i0 j0 n1 n2.  Returns the ints written, or -1 with the message in err. */
#include "mesh_cuts.h"

static mc_mesh M;

int probe_mesh_cuts(int nlev, const int *nx, const int *disp, const int *rootNx, int nslab, const int *cuts, int periodic3,
                    int *out, int nout, char *err, int nerr)
{
  mc_level lev[MC_MAXLEV];
  int eq[MC_MAXSLAB + 1], n = 0, s, l, q;
  if (nlev > MC_MAXLEV || nslab > MC_MAXSLAB || nslab < 1) return -1;
  for (l = 0; l < nlev; l++) for (q = 0; q < 3; q++) { lev[l].Nx[q] = nx[3*l + q]; lev[l].disp[q] = disp[3*l + q]; }
  if (!cuts) { mc_equal_cuts(rootNx[2], nslab, eq); cuts = eq; }
  if (mc_build(&M, nlev, lev, rootNx, nslab, cuts, periodic3, err, nerr)) return -1;
#define PUT(v) do { if (n >= nout) return -1; out[n++] = (v); } while (0)
  for (s = 0; s < nslab; s++) {
    const mc_slab *S = &M.slab[s];
    PUT(S->nl);
    for (l = 0; l < S->nl; l++) { PUT(S->piece[l].k0); PUT(S->piece[l].k1); PUT(S->piece[l].lo); PUT(S->piece[l].hi); }
    for (l = 0; l + 1 < S->nl; l++) {
      int w[21];
      mc_link_ints(&S->link[l], w);
      for (q = 0; q < 21; q++) PUT(w[q]);
      PUT(S->link[l].corr_to[0]); PUT(S->link[l].corr_to[1]);
    }
    PUT(S->ncorr_in);
    for (l = 0; l < S->ncorr_in; l++) {
      const mc_corr_in *c = &S->corr_in[l];
      PUT(c->level); PUT(c->side); PUT(c->src); PUT(c->i0); PUT(c->j0); PUT(c->n1); PUT(c->n2);
    }
  }
  return n;
}
