/* mesh_cuts.h -- the arithmetic of a Mesh whose levels are all cut at the same root x3 planes (plain C, no device).
 *
 * Slab s owns the root planes [K_s, K_s+1) and, of level l, the zones lying over them.  Restriction, the radiation hand-off and
 * prolongation then stay inside a slab; what crosses slabs is the x3 halo of every level and the flux correction of the one
 * parent plane that lies across a cut from the child's boundary.  ONE Domain per level (level l is entry l).  The same rules as
 * config.mesh_slabs:
 *   - a piece thinner than nghost is an error that names the level, the slab and the cut;
 *   - bc[4] / bc[5] of a piece become AA_BC_NONE on interior cuts (lo / hi below name the neighbour slab);
 *   - a periodic root wraps (the root level only).
 * Every function returns 0, or -1 with a message in err.
 */
#ifndef AA_MESH_CUTS_H
#define AA_MESH_CUTS_H
#include <stdio.h>
#include <string.h>

#define MC_NGHOST  4
#define MC_MAXLEV  16
#define MC_MAXSLAB 64

typedef struct mc_level { int Nx[3]; int disp[3]; } mc_level;      /* zones and displacement in zones of the level (root: disp 0) */

typedef struct mc_piece {       /* level l on slab s */
  int k0, k1;                   /* planes [k0, k1) in zones of the level, root-relative as disp; k1 <= k0: no zones */
  int lo, hi;                   /* neighbour slab below / above that continues the level (-1: the level's own boundary) */
} mc_piece;

typedef struct mc_link {        /* level l+1 on level l inside a slab: the 21 ints of aa_mesh_create_local, plus corr_to */
  int cs[3], n[3], prol[6], corr[6], cdisp[3];
  int corr_to[2];               /* x3 sides: slab owning the parent plane outside (-1: local or no boundary) */
} mc_link;

typedef struct mc_corr_in {     /* a flux correction arriving from a neighbour's child piece */
  int level, side, src;         /* level of the parent, side of the child boundary (0 lower / 1 upper), source slab */
  int i0, j0, n1, n2;           /* region of the parent plane, local indices incl. ghosts */
} mc_corr_in;

typedef struct mc_slab {
  int nl;                                   /* levels with zones on this slab, root first */
  mc_piece piece[MC_MAXLEV];
  mc_link link[MC_MAXLEV];                  /* link[l]: level l+1 on level l, l + 1 < nl */
  int ncorr_in; mc_corr_in corr_in[2*MC_MAXLEV];
} mc_slab;

typedef struct mc_mesh {
  int nslab, nlev, rootNx[3];
  int cuts[MC_MAXSLAB + 1];
  mc_level lev[MC_MAXLEV];
  mc_slab slab[MC_MAXSLAB];
} mc_mesh;

/* init_mesh.c:583-620: Nx3/N planes each, the remainder to the first slabs */
static inline void mc_equal_cuts(int n3, int nslab, int *cuts)
{
  int s, k = 0;
  cuts[0] = 0;
  for (s = 0; s < nslab; s++) { k += n3/nslab + (s < n3 % nslab ? 1 : 0); cuts[s + 1] = k; }
}

static inline int mc_check_cuts(int n3, int nslab, const int *cuts, char *err, int nerr)
{
  int s, bad = (nslab < 1 || nslab > MC_MAXSLAB);
  if (!bad) bad = (cuts[0] != 0 || cuts[nslab] != n3);
  for (s = 0; s < nslab && !bad; s++) if (cuts[s + 1] - cuts[s] < MC_NGHOST) bad = 1;
  if (bad) { if (err) snprintf(err, (size_t)nerr, "bad x3 cuts for %d slabs of %d root planes (0 = K_0 < .. < K_N = Nx3, slabs need >= %d root planes)", nslab, n3, MC_NGHOST); return -1; }
  return 0;
}

/* the planes of ONE level (Nx3 zones displaced by kdisp, zones of the level) over the root planes [cuts[s], cuts[s+1]) */
static inline int mc_span(int level, int Nx3, int kdisp, int s, const int *cuts, int *k0, int *k1, char *err, int nerr)
{
  const int f = 1 << level, d3 = level ? kdisp : 0;
  const int a = f*cuts[s], b = f*cuts[s + 1];
  *k0 = d3 > a ? d3 : a; *k1 = (d3 + Nx3) < b ? (d3 + Nx3) : b;
  if (*k1 <= *k0) { *k0 = *k1 = 0; return 0; }
  if (*k1 - *k0 < MC_NGHOST) {
    if (err) snprintf(err, (size_t)nerr, "level %d on slab %d is %d planes thin, fewer than nghost = %d (root cut at plane %d): choose other cuts",
                      level, s, *k1 - *k0, MC_NGHOST, (*k0 == d3) ? cuts[s + 1] : cuts[s]);
    return -1;
  }
  return 0;
}

static inline int mc_build(mc_mesh *m, int nlev, const mc_level *lev, const int rootNx[3], int nslab, const int *cuts, int periodic3,
                           char *err, int nerr)
{
  int s, l, d;
  if (nlev < 1 || nlev > MC_MAXLEV) { if (err) snprintf(err, (size_t)nerr, "%d levels", nlev); return -1; }
  if (mc_check_cuts(rootNx[2], nslab, cuts, err, nerr)) return -1;
  memset(m, 0, sizeof *m);
  m->nslab = nslab; m->nlev = nlev;
  for (d = 0; d < 3; d++) m->rootNx[d] = rootNx[d];
  for (s = 0; s <= nslab; s++) m->cuts[s] = cuts[s];
  for (l = 0; l < nlev; l++) { m->lev[l] = lev[l]; if (l == 0) m->lev[0].disp[0] = m->lev[0].disp[1] = m->lev[0].disp[2] = 0; }
  for (s = 0; s < nslab; s++) {
    mc_slab *S = &m->slab[s];
    S->nl = 0;
    for (l = 0; l < nlev; l++) {
      mc_piece *p = &S->piece[l];
      const int thin = mc_span(l, m->lev[l].Nx[2], m->lev[l].disp[2], s, cuts, &p->k0, &p->k1, err, nerr);
      p->lo = p->hi = -1;
      if (S->nl < l) { p->k0 = p->k1 = 0; if (thin && err) err[0] = 0; continue; }     /* without the parent, no finer level either */
      if (thin) return -1;
      if (p->k1 <= p->k0) continue;
      S->nl = l + 1;
    }
  }
  for (s = 0; s < nslab; s++) {
    mc_slab *S = &m->slab[s];
    for (l = 0; l < S->nl; l++) {
      mc_piece *p = &S->piece[l];
      const int d3 = m->lev[l].disp[2];
      if (p->k0 > d3) p->lo = s - 1;
      else if (l == 0 && periodic3 && nslab > 1) p->lo = nslab - 1;
      if (p->k1 < d3 + m->lev[l].Nx[2]) p->hi = s + 1;
      else if (l == 0 && periodic3 && nslab > 1) p->hi = 0;
    }
    for (l = 0; l + 1 < S->nl; l++) {
      const mc_piece *P = &S->piece[l], *C = &S->piece[l + 1];
      const mc_level *Pg = &m->lev[l], *Cg = &m->lev[l + 1];
      const int irefine = 1 << (l + 1);
      mc_link *L = &S->link[l];
      L->corr_to[0] = L->corr_to[1] = -1;
      for (d = 0; d < 3; d++) {
        const int pd = (d < 2) ? Pg->disp[d] : P->k0, pn = (d < 2) ? Pg->Nx[d] : P->k1 - P->k0;
        const int cd = (d < 2) ? Cg->disp[d] : C->k0, cn = (d < 2) ? Cg->Nx[d] : C->k1 - C->k0;
        const int a = cd/2 - pd, b = (cd + cn)/2 - pd;
        const int glo = Cg->disp[d], ghi = Cg->disp[d] + Cg->Nx[d];
        const int at_lo = (cd == glo) && glo != 0;                                  /* a fine/coarse boundary of the LEVEL */
        const int at_hi = (cd + cn == ghi) && (ghi/irefine != rootNx[d]);
        L->cs[d] = a + MC_NGHOST; L->n[d] = b - a; L->cdisp[d] = cd - 2*pd;
        L->prol[2*d] = at_lo; L->prol[2*d + 1] = at_hi;
        L->corr[2*d] = L->corr[2*d + 1] = 0;
        if (at_lo) { if (a > 0 || d < 2) L->corr[2*d] = 1; else L->corr_to[0] = s - 1; }
        if (at_hi) { if (b < pn || d < 2) L->corr[2*d + 1] = 1; else L->corr_to[1] = s + 1; }
      }
    }
    S->ncorr_in = 0;
    for (l = 0; l < S->nl && l + 1 < nlev; l++) {
      const mc_piece *P = &S->piece[l];
      const mc_level *Pg = &m->lev[l], *Cg = &m->lev[l + 1];
      const int irefine = 1 << (l + 1), ghi = Cg->disp[2] + Cg->Nx[2];
      mc_corr_in c;
      c.level = l;
      c.i0 = Cg->disp[0]/2 - Pg->disp[0] + MC_NGHOST; c.j0 = Cg->disp[1]/2 - Pg->disp[1] + MC_NGHOST;
      c.n1 = Cg->Nx[0]/2; c.n2 = Cg->Nx[1]/2;
      /* the child level starts exactly at my upper cut: my top plane lies outside its lower boundary */
      if (Cg->disp[2] == 2*P->k1 && Cg->disp[2] != 0 && s + 1 < nslab && m->slab[s + 1].nl > l + 1) {
        c.side = 0; c.src = s + 1; S->corr_in[S->ncorr_in++] = c;
      }
      if (ghi == 2*P->k0 && ghi/irefine != rootNx[2] && s > 0 && m->slab[s - 1].nl > l + 1) {
        c.side = 1; c.src = s - 1; S->corr_in[S->ncorr_in++] = c;
      }
    }
  }
  return 0;
}

/* link l of slab s in the layout aa_mesh_create_local takes */
static inline void mc_link_ints(const mc_link *L, int *q)
{
  int d;
  for (d = 0; d < 3; d++) { q[d] = L->cs[d]; q[3 + d] = L->n[d]; q[18 + d] = L->cdisp[d]; }
  for (d = 0; d < 6; d++) { q[6 + d] = L->prol[d]; q[12 + d] = L->corr[d]; }
}

#endif
