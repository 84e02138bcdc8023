/* tests/fixtures/ion_matrix.c -- a USER problem file written against the reference's public problem-file API
 * (prototypes.h:199-205; add_radplane_3d, ionradiation/prototypes.h:66), used to pin the reference's per-zone chemistry
 * of the radiation sub-cycle (ionrad_3d.c:70-590) on a state DESIGNED to reach every branch of it.  Not derived from any
 * reference problem file.
 *
 * Every active zone is set from integer patterns of its indices alone (no cc_pos, no random numbers); the factors cycle
 * with co-prime periods so that they combine:
 *   temperature (9)   E < ke, E == ke, 5, 50, 130, 1000, 9000, 3e4, 3e6 K -- below the floor, between the floor, the 100 K
 *                     switch of the recombination cooling and the Lyman-alpha cut-off at 158.8 K, above the ceiling
 *   neutral part (7)  s/d = 1, 0.5, 1e-3, 1e-6, 1.2 (above d), -0.1 (below the floor), and s = 1.00005 d_nlim (held)
 *   density (2)       d 1e-4 on either side of d_nlo (d_nlim = d IONFRACFLOOR for the one, d_nlo for the other) in the first half
 *                     of every ray, both 10 times denser in the second half
 *   momentum (2)      zero, or 1 km/s shared out over the three directions
 * The first half is thin enough that the rays cross it and end at different depths behind it: lit and dark zones occur in
 * every class.  (The dense half also carries the largest energies of the grid, which keeps what a zone AT the temperature
 * floor gains or not in one sub-cycle -- see below -- small against the scale whole-run comparisons are made on.)  The first zone of every ray is set apart as a window: neutral, at rest, 50 K, dense enough (tau = 3.7)
 * to take most of the flux.  It is the zone that heats fastest, so that no zone sitting exactly AT the temperature floor --
 * where "cold" is decided in the last bit -- sets the thermal time-step limit.
 * tests/ionmatrix.py states the same expressions in numpy, operation by operation.
 * Keys: <problem> n_H, flux, d_nlo (the reference's lower limit of the neutral density on this grid, handed in so that
 * this file does not restate how ionrad.c derives it); <ionradiation> m_H, mu, alpha_C, k_B.
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
  static const Real Tpat[9] = {-5.0, 0.0, 5.0, 50.0, 130.0, 1000.0, 9000.0, 3.0e4, 3.0e6};
  static const Real spat[6] = {1.0, 0.5, 1.0e-3, 1.0e-6, 1.2, -0.1};
  static const Real dpat[2] = {1.0e-4, 2.0e-3};
  Real n_H = par_getd("problem", "n_H"), flux = par_getd("problem", "flux"), d_nlo = par_getd("problem", "d_nlo");
  Real m_H = par_getd("ionradiation", "m_H"), mu = par_getd("ionradiation", "mu");
  Real alpha_C = par_getd("ionradiation", "alpha_C"), k_B = par_getd("ionradiation", "k_B");
  Real v0 = 1.0e5;
  for (k = pG->ks; k <= pG->ke; k++) for (j = pG->js; j <= pG->je; j++) for (i = pG->is; i <= pG->ie; i++) {
    int a = i - pG->is, b = j - pG->js, c = k - pG->ks;
    int tI = (a + 2*b + 5*c) % 9, sI = (a + 3*b + c) % 7, dI = (a + b + c) % 2, mI = (a/2 + c) % 2;
    Real d, d_nlim, s, n_e, x, muq, e_th, M1, M2, M3, ke;
    if (a == 0) { tI = 3; sI = 0; mI = 0; }       /* the window: the first zone of every ray */
    d = n_H*m_H*((a == 0) ? 2.0e-2 : (2*a >= pG->Nx[0]) ? 10.0*dpat[dI] : dpat[dI]);
    d_nlim = d*1.0e-4;
    if (d_nlo < d_nlim) d_nlim = d_nlo;
    s = (sI < 6) ? spat[sI]*d : 1.00005*d_nlim;
    n_e = (d - s)/m_H + d*alpha_C/(14.0*m_H);
    x = n_e/(s/m_H + (d - s)/m_H);
    muq = x*0.5*m_H + (1.0 - x)*mu;
    e_th = d*(Tpat[tI]*k_B/(muq*Gamma_1));
    M1 = (Real)mI*d*v0; M2 = -0.5*M1; M3 = 0.25*M1;
    ke = 0.5*(M1*M1 + M2*M2 + M3*M3)/d;
    pG->U[k][j][i].d = d;
    pG->U[k][j][i].M1 = M1; pG->U[k][j][i].M2 = M2; pG->U[k][j][i].M3 = M3;
    pG->U[k][j][i].E = ke + e_th;
    pG->U[k][j][i].s[0] = s;
  }
  add_radplane_3d(pG, -1, flux);
}

void problem_write_restart(MeshS *pM, FILE *fp) { return; }
void problem_read_restart(MeshS *pM, FILE *fp) { return; }
ConsFun_t get_usr_expr(const char *expr) { return NULL; }
VOutFun_t get_usr_out_fun(const char *name) { return NULL; }
void Userwork_in_loop(MeshS *pM) { return; }
void Userwork_after_loop(MeshS *pM) { return; }
