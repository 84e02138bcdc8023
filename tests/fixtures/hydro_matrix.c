/* tests/fixtures/hydro_matrix.c -- a USER problem file written against the reference's public problem-file API
 * (prototypes.h:199-205), used to pin the reference's hydro step on a state DESIGNED to reach every branch of it: the two
 * supersonic returns and the HLLE fallback of the Roe solver (roe.c:215-286), the outcomes of the slope limiter and the
 * monotonicity clamps, the tracing branches of lr_states_plm.c / lr_states_ppm.c, the H-correction on both sides of
 * MAX(|ev|, etah), and (where asked for) the pressure floor of Cons1D_to_Prim1D.  Not derived from any reference problem file.
 *
 * Every active zone is set from integer patterns of its ROOT-zone indices alone (no cc_pos, no random numbers): a zone of a
 * refined level takes the indices of the root zone it lies in, so the fine zones of a coarse one are exact copies.
 *   blocks    of 3 root zones along each axis.  The velocity along an axis is boosted block by block through the cycle
 *             -1, +1, 0, +1 times vb (2.6, 2.4, 2.8 along x1, x2, x3: twice the sound speed), the cycles starting at
 *             different blocks along the three axes: blocks receding from each other at four and at two sound speeds, blocks running
 *             into gas at rest, supersonic blocks of either sign along each axis
 *   vacuum    every fifth block along the diagonal is a near-vacuum block: density dvac, pressure pvac times the quiet gas'.
 *             pvac < 0 puts the total energy below the kinetic energy there (what an overshoot leaves behind): the
 *             pressure floor acts from the first step
 *   quiet gas density 1 ... 1.5, pressure 1 ... 1.2 and a shear of a few per cent of the sound speed in all three velocities,
 *             by patterns of co-prime periods, different per direction
 *   scalar    (configurations with NSCALARS > 0) s = d*r, the concentration r = 0.125 ... 0.875 by a pattern of period 7 (co-prime
 *             to the block cycle, another value across every face along each axis, exact in binary)
 * tests/hydromatrix.py states the same expressions in numpy, operation by operation.
 * Keys: <problem> dvac, pvac (gamma is read by the reference's main); seed (optional, default 0): a seed other than 0 moves every
 * conserved variable (the scalar included) of every zone by one unit in the last place, up or down by a shift-register sequence -- the 1-ulp twins by
 * which tests/golden/make_golden_hydromatrix.py measures how well conditioned a run of the reference is.
 */
#include <math.h>
#include <stdio.h>
#include "defs.h"
#include "athena.h"
#include "globals.h"
#include "prototypes.h"

void problem(DomainS *pDomain)
{
  GridS *pG = pDomain->Grid;
  int i, j, k;
  const int lev = pDomain->Level;
  static const Real seq[4] = {-1.0, 1.0, 0.0, 1.0};
  static const Real vb[3] = {2.6, 2.4, 2.8};
  Real dvac = par_getd("problem", "dvac"), pvac = par_getd("problem", "pvac");
  const int seed = par_geti_def("problem", "seed", 0);
  unsigned long long rs = 88172645463325252ULL*(unsigned long long)(seed + 7*lev + 1);
  for (k = pG->ks; k <= pG->ke; k++) for (j = pG->js; j <= pG->je; j++) for (i = pG->is; i <= pG->ie; i++) {
    int a = (i - pG->is + pG->Disp[0]) >> lev, b = (j - pG->js + pG->Disp[1]) >> lev, c = (k - pG->ks + pG->Disp[2]) >> lev;
    int A = a/3, B = b/3, C = c/3;
    Real d = 1.0 + 0.125*(Real)((a + 2*b + 3*c) % 5);
    Real p = 1.0 + 0.1*(Real)((2*a + b + c) % 3);
    Real v1 = 0.05*((Real)((3*a + 5*b + 7*c) % 5) - 2.0);
    Real v2 = 0.04*((Real)((a + 2*b + 3*c) % 7) - 3.0);
    Real v3 = 0.03*((Real)((2*a + b + 4*c) % 3) - 1.0);
    if ((A + B + C) % 5 == 1) { d = dvac*d; p = pvac*p; }
    v1 = v1 + vb[0]*seq[(A + 1) % 4];
    v2 = v2 + vb[1]*seq[(B + 3) % 4];
    v3 = v3 + vb[2]*seq[C % 4];
    pG->U[k][j][i].d = d;
    pG->U[k][j][i].M1 = d*v1; pG->U[k][j][i].M2 = d*v2; pG->U[k][j][i].M3 = d*v3;
    pG->U[k][j][i].E = p/Gamma_1 + 0.5*d*(v1*v1 + v2*v2 + v3*v3);
#if (NSCALARS > 0)
    pG->U[k][j][i].s[0] = d*(0.125 + 0.125*(Real)((a + 3*b + 5*c) % 7));
#endif
    if (seed != 0) {
      Real *q = (Real*)&(pG->U[k][j][i]); int n;
      for (n = 0; n < 5 + NSCALARS; n++) { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; q[n] = nextafter(q[n], (rs & 1024) ? 1.0e300 : -1.0e300); }
    }
  }
}

void problem_write_restart(MeshS *pM, FILE *fp) { return; }
void problem_read_restart(MeshS *pM, FILE *fp) { return; }
ConsFun_t get_usr_expr(const char *expr) { return NULL; }
VOutFun_t get_usr_out_fun(const char *name) { return NULL; }
void Userwork_in_loop(MeshS *pM) { return; }
void Userwork_after_loop(MeshS *pM) { return; }
