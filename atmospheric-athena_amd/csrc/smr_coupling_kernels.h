// smr_coupling_kernels.h -- the three kernels of smr.hip that couple two levels of a 3-D Mesh and change with the step's dt or
// must not run behind a stop: restriction, flux correction, the snapshot for the prolongation.  Included by smr.hip inside its
// unnamed namespace (Link, fld).  No include guard: compiled twice --
//   as it stands          k_restrict(f, c, L, varmask), k_flux_correct(f, c, L, dim_arg, nvar, dt), k_box_copy(c, L, box)
//   AA_CLOCK_ENTRY        k_restrict_dc(.., rc), k_flux_correct_dc(.., nvar, rc), k_box_copy_dc(.., rc): a step queued by
//                         aa_mesh_run_3d.  The clock (hydro3d_launch.h Run3D, in device memory; any Grid's of the Mesh's array:
//                         time, dt, `live` and `stepped` are the same in all) is read at the top, as the *_dc entries of
//                         hydro_kernels.hip do.  Restriction OVERWRITES the parent with a function of the child, but the flux
//                         correction ADDS to the parent: behind the stop (`live` = 0) both return before any store, and dt is the
//                         clock's.  The snapshot stands behind k3d_mesh_advance, which has already written the NEXT step's
//                         `live`: it asks `stepped`, whether the step in front of that kernel was taken (smr.hip
//                         mesh_queue_step_3d says why a snapshot behind a stop must not be retaken).
// Below the opening brace the two are one text.

// ---- restriction: 2x2x2 fine zones -> one parent zone, summed as smr.c:1391-1458 -------------
// varmask bit v = restrict variable v (RestrictCorrect: all; ionradRestrictCorrect: E and s0)
__global__ void __launch_bounds__(256)
#ifdef AA_CLOCK_ENTRY
k_restrict_dc(DevGrid f, DevGrid c, Link L, unsigned varmask, const Run3D *rc)
{
  if (!rc->c.live) return;
#else
k_restrict(DevGrid f, DevGrid c, Link L, unsigned varmask)
{
#endif
  const long n = (long)L.n[0]*L.n[1]*L.n[2];
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= n) return;
  const int a = (int)(lin % L.n[0]), b = (int)((lin / L.n[0]) % L.n[1]), cc = (int)(lin / ((long)L.n[0]*L.n[1]));
  const long mc = (long)(L.cs[2] + cc)*c.sK + (long)(L.cs[1] + b)*c.sJ + (L.cs[0] + a);
  const long mf = (long)(f.ks + 2*cc)*f.sK + (long)(f.js + 2*b)*f.sJ + (f.is + 2*a);
  for (int v = 0; v < 6; v++) {
    if (!(varmask >> v & 1u)) continue;
    const Real *q = fld(f, f.U, v) + mf;
    Real s = q[0] + q[1];
    s += q[f.sJ] + q[f.sJ + 1];
    s += q[f.sK] + q[f.sK + 1] + q[f.sK + f.sJ] + q[f.sK + f.sJ + 1];
    s *= 0.125;
    fld(c, c.U, v)[mc] = s;
  }
}

// ---- flux correction (smr.c:1277-1340) on the parent zones just outside the child, one side per
// launch; the child's flux through a parent face is the average of its 2x2 faces (:1464-1640) ----
__global__ void __launch_bounds__(256)
#ifdef AA_CLOCK_ENTRY
k_flux_correct_dc(DevGrid f, DevGrid c, Link L, int dim_arg, int nvar, const Run3D *rc)
{
  if (!rc->c.live) return;
  const Real dt = rc->c.dt;
#else
k_flux_correct(DevGrid f, DevGrid c, Link L, int dim_arg, int nvar, Real dt)
{
#endif
  // dim_arg < 0: all sides in one launch, side = blockIdx.y (the sides correct disjoint parent zones: the zone outside each face)
  const int dim = (dim_arg >= 0) ? dim_arg : (int)blockIdx.y;
  if (dim_arg < 0 && !L.corr[dim]) return;
  const int d = dim >> 1, d1 = (d == 0) ? 1 : 0, d2 = (d == 2) ? 1 : 2;      // fast, slow transverse
  const long n = (long)L.n[d1]*L.n[d2];
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= n) return;
  const int a = (int)(lin % L.n[d1]), b = (int)(lin / L.n[d1]);
  const long sc[3] = {1, c.sJ, c.sK}, sf[3] = {1, f.sJ, f.sK};
  const int flo[3] = {f.is, f.js, f.ks}, fhi[3] = {f.ie, f.je, f.ke};
  int ic[3]; ic[d1] = L.cs[d1] + a; ic[d2] = L.cs[d2] + b;
  Real q;
  long mface_c, mcell, mface_f;
  if (dim & 1) { ic[d] = L.ce[d] + 1; q =  (dt/c.dx[d]); }
  else         { ic[d] = L.cs[d] - 1; q = -(dt/c.dx[d]); }
  mcell = ic[2]*sc[2] + ic[1]*sc[1] + ic[0];
  ic[d] = (dim & 1) ? L.ce[d] + 1 : L.cs[d];
  mface_c = ic[2]*sc[2] + ic[1]*sc[1] + ic[0];
  {
    int jf[3]; jf[d1] = flo[d1] + 2*a; jf[d2] = flo[d2] + 2*b; jf[d] = (dim & 1) ? fhi[d] + 1 : flo[d];
    mface_f = jf[2]*sf[2] + jf[1]*sf[1] + jf[0];
  }
  for (int v = 0; v < nvar; v++) {
    const Real mine = fld(c, c.F, d*6 + v)[mface_c];
    const Real *qf = fld(f, f.F, d*6 + v) + mface_f;
    Real fine = qf[0] + qf[sf[d1]];
    fine += qf[sf[d2]] + qf[sf[d2] + sf[d1]];
    fine *= 0.25;
    fld(c, c.U, v)[mcell] -= q*(mine - fine);
  }
}

// snapshot of the parent zones cs-3 .. ce+3 around the child, taken when the parent "sends"
// (smr.c:2397-2470: before the parent's own ghost zones are refreshed in the same call)
__global__ void __launch_bounds__(256)
#ifdef AA_CLOCK_ENTRY
k_box_copy_dc(DevGrid c, Link L, Real *box, const Run3D *rc)
{
  if (!rc->stepped) return;
#else
k_box_copy(DevGrid c, Link L, Real *box)
{
#endif
  const int b0 = L.n[0] + 6, b1 = L.n[1] + 6, b2 = L.n[2] + 6;
  const long nb = (long)b0*b1*b2;
  const long lin = (long)blockIdx.x*blockDim.x + threadIdx.x;
  if (lin >= nb) return;
  const int i = (int)(lin % b0), j = (int)((lin / b0) % b1), k = (int)(lin / ((long)b0*b1));
  const long m = (long)(L.cs[2] - 3 + k)*c.sK + (long)(L.cs[1] - 3 + j)*c.sJ + (L.cs[0] - 3 + i);
  for (int v = 0; v < 6; v++) box[(long)v*nb + lin] = fld(c, c.U, v)[m];
}
