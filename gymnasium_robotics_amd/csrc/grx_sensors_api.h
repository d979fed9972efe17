// grx_sensors_api.h -- the C ABI of the sensor block (include/grx_capi.h grx_sim_step_sns / grx_sim_sensors_layout).  A FRAGMENT of the API section of grx_kernels.hip (it uses
// that section's grx_model, fail, HIP_OK and grx_sim_step_impl), as grx_rays_api.h is; the routines are csrc/grx_sim_sensors.h, the kernels the
// instances of grx_sim_step_kernel / grx_sim_lane_kernel with all five blocks (the rows simsns / simsnsprm of GRX_SIM_UNITS, units GRX_TU_SIMSNS / GRX_TU_SIMSNSPRM).

// The host table, checked on the host: a known type, an object of the kind the type reads with an id in range, rows that tile [0, ndata) in order.
static int grx_sensor_table_check(const grx_model* m, const grx_sim_sensors* s) {
  const GrxModel& g = m->dev;
  const int k_jt = grx_find_table(m->pm, "jnt_type");
  const int32_t* jtype = k_jt >= 0 ? m->pm.i.data() + m->pm.off[k_jt] : nullptr;
  int adr = 0;
  for (int k = 0; k < s->nsensor; k++) {
    const int type = s->spec[4 * k], objtype = s->spec[4 * k + 1], id = s->spec[4 * k + 2];
    const std::string who = "grx_sim_step_sns: sensor " + std::to_string(k);
    if (type < 0 || type >= GRX_SNS_NTYPE) return fail(who + " has the unknown type " + std::to_string(type));
    if (objtype < 0 || objtype >= GRX_SNS_NOBJ) return fail(who + " has the unknown object type " + std::to_string(objtype));
    const bool joint = type == GRX_SNS_JOINTPOS || type == GRX_SNS_JOINTVEL || type == GRX_SNS_JOINTACTFRC, act = type >= GRX_SNS_ACTUATORPOS && type <= GRX_SNS_ACTUATORFRC;
    const bool site_only = type == GRX_SNS_VELOCIMETER || type == GRX_SNS_GYRO || type == GRX_SNS_ACCELEROMETER || type == GRX_SNS_FORCE || type == GRX_SNS_TORQUE;
    const bool ok = joint ? objtype == GRX_SNS_OBJ_JOINT : act ? objtype == GRX_SNS_OBJ_ACTUATOR : site_only ? objtype == GRX_SNS_OBJ_SITE : (objtype == GRX_SNS_OBJ_SITE || objtype == GRX_SNS_OBJ_XBODY);
    if (!ok) return fail(who + ": type " + std::to_string(type) + " does not read an object of type " + std::to_string(objtype) + " (joint types read joints, actuator types actuators, velocimeter / gyro / accelerometer / force / torque sites, the frame types sites or xbodies)");
    const int lim = objtype == GRX_SNS_OBJ_JOINT ? g.njnt : objtype == GRX_SNS_OBJ_ACTUATOR ? g.nu : objtype == GRX_SNS_OBJ_SITE ? g.nsite : g.nbody;
    if (id < 0 || id >= lim) return fail(who + ": object id " + std::to_string(id) + " is outside [0, " + std::to_string(lim) + ")");
    if (joint && (!jtype || id >= m->pm.cnt[k_jt] || jtype[id] < 2)) return fail(who + ": joint " + std::to_string(id) + " is a free or ball joint (the joint types read hinge and slide joints)");
    if (s->spec[4 * k + 3] != adr) return fail(who + ": adr = " + std::to_string(s->spec[4 * k + 3]) + ", the rows before it end at " + std::to_string(adr) + " (the rows tile [0, ndata) in sensor order)");
    if (!(s->cutoff[k] >= 0.0f) || !std::isfinite(s->cutoff[k])) return fail(who + ": cutoff is negative or not finite");
    adr += grx_sensor_dim(type);
  }
  if (adr != s->ndata) return fail("grx_sim_step_sns: the rows of the table end at " + std::to_string(adr) + ", ndata = " + std::to_string(s->ndata));
  return 0;
}

// the device copy of a checked table: made once per distinct content (one blocking upload) and kept with the handle, as grx_ray_site_list keeps its lists -- a simulation
// passes the same table in every launch, so every launch after the first only enqueues.  The handle keeps the 16 most recent tables.
static int grx_sensor_table(const grx_model* m, const grx_sim_sensors* s, const int** spec, const float** cutoff) {
  const size_t n = (size_t)s->nsensor;
  std::vector<int> key(5 * n);
  memcpy(key.data(), s->spec, sizeof(int) * 4 * n);
  memcpy(key.data() + 4 * n, s->cutoff, sizeof(float) * n);
  std::lock_guard<std::mutex> lk(m->ray_mu);
  int* d = nullptr;
  for (auto& e : m->sensor_tables) if (e.first == key) d = e.second;
  if (!d) {
    if (grx_sensor_table_check(m, s)) return -1;
    HIP_OK(hipSetDevice(m->device));
    if (m->sensor_tables.size() >= 16) {      // the oldest table goes: hipFree waits for the launches that may still read it
      (void)hipFree(m->sensor_tables.front().second);
      m->sensor_tables.erase(m->sensor_tables.begin());
    }
    HIP_OK(hipMalloc(&d, sizeof(int) * key.size()));
    if (hipMemcpy(d, key.data(), sizeof(int) * key.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return fail("grx_sim_step_sns: upload of the sensor table failed"); }
    m->sensor_tables.emplace_back(std::move(key), d);
  }
  *spec = d; *cutoff = (const float*)(d + 4 * n);
  return 0;
}

// What the two entries that take a sensor table do with it.  *has <- the block carries data and sensors (one that does not launches what the call without it launches).
// Then the checks, *nft <- the number of force / torque rows (wrn: the caller serves them; otherwise they are refused, before anything is uploaded), and *d <- the block as
// the kernels see it, with the handle's device tables in place of the caller's host tables.
static int grx_sim_sensor_block(const grx_model* m, const grx_sim_sensors* sns, bool wrn, GrxSimSensors* d, int* nft, bool* has) {
  *nft = 0;
  *has = sns && sns->data && sns->nsensor != 0;
  if (!*has) return 0;
  if (sns->nsensor < 0 || sns->ndata < 1) return fail("grx_sim_step_sns: nsensor < 0 or ndata < 1 with a data buffer set");
  if (!sns->spec || !sns->cutoff) return fail("grx_sim_step_sns: null spec / cutoff table (host arrays [nsensor, 4] and [nsensor])");
  if (!m) return fail("grx_sim_step: null model");
  for (int k = 0; k < sns->nsensor; k++) *nft += sns->spec[4 * k] == GRX_SNS_FORCE || sns->spec[4 * k] == GRX_SNS_TORQUE;
  if (*nft && !wrn) return fail("grx_sim_step_sns: the table holds " + std::to_string(*nft) + " force / torque sensor(s), which read cfrc_int: grx_sim_step_wrn is the call that serves them");
  memset(d, 0, sizeof(*d));
  d->nsensor = sns->nsensor; d->ndata = sns->ndata; d->data = sns->data;
  return grx_sensor_table(m, sns, &d->spec, &d->cutoff);
}
// The stepper with the fifth block.  params, dyn, con and frc may be null and mean what they mean to grx_sim_step_frc; a block without data or without sensors launches what
// that call launches for the other arguments.
extern "C" int grx_sim_step_sns(const grx_model* m, const grx_sim_params* p, const grx_sim_buffers* buf, const grx_sim_dynamics* dyn, const grx_sim_contacts* con, const grx_sim_applied* frc, const grx_sim_sensors* sns,
                                int n_worlds, int nstep, int forward_only, void* stream) {
  if (!sns) return fail("grx_sim_step_sns: null sensor block (grx_sim_step_frc is the call without one)");
  const GrxModel* desc;
  if (grx_sim_params_desc(m, p, n_worlds, &desc)) return -1;
  GrxSimStepArgs s = {m, buf, dyn, n_worlds, nstep, forward_only, stream, desc, con, frc};
  GrxSimSensors d; int nft; bool has;
  if (grx_sim_sensor_block(m, sns, false, &d, &nft, &has)) return -1;
  if (has) s.sns = &d;
  return grx_sim_step_impl(s);
}
// The stepper with the sixth block (body wrenches, csrc/grx_sim_wrench.h).  sns and wrn may be null; with nothing of the block requested -- no pointer set, no force / torque
// row in the table -- the launch is grx_sim_step_sns's (or, without sensors, grx_sim_step_frc's).
extern "C" int grx_sim_step_wrn(const grx_model* m, const grx_sim_params* p, const grx_sim_buffers* buf, const grx_sim_dynamics* dyn, const grx_sim_contacts* con, const grx_sim_applied* frc, const grx_sim_sensors* sns,
                                const grx_sim_wrenches* wrn, int n_worlds, int nstep, int forward_only, void* stream) {
  const GrxModel* desc;
  if (grx_sim_params_desc(m, p, n_worlds, &desc)) return -1;
  GrxSimStepArgs s = {m, buf, dyn, n_worlds, nstep, forward_only, stream, desc, con, frc};
  GrxSimSensors d; GrxSimWrenches r; int nft; bool has;
  if (grx_sim_sensor_block(m, sns, true, &d, &nft, &has)) return -1;
  if (has) s.sns = &d;
  memset(&r, 0, sizeof(r));
  if (wrn) { r.cfrc_ext = wrn->cfrc_ext; r.cfrc_int = wrn->cfrc_int; r.cacc = wrn->cacc; r.subtree_com = wrn->subtree_com; }
  r.nft = nft;
  if (r.cfrc_ext || r.cfrc_int || r.cacc || r.subtree_com || nft) s.wrn = &r;
  return grx_sim_step_impl(s);
}
// sizeof(grx_sim_wrenches) and the byte offset of every member, in declaration order: what _native.SimWrenchesStruct must mirror (host only)
extern "C" int grx_sim_wrenches_layout(long long* out, int cap) {
  const grx_sim_wrenches* z = nullptr;
#define OFF(f) (long long)((const char*)&z->f - (const char*)z)
  const long long v[] = {(long long)sizeof(grx_sim_wrenches), OFF(cfrc_ext), OFF(cfrc_int), OFF(cacc), OFF(subtree_com)};
#undef OFF
  const int n = (int)(sizeof(v) / sizeof(v[0]));
  if (out) for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
  return n;
}
// sizeof(grx_sim_sensors) and the byte offset of every member, in declaration order: what _native.SimSensorsStruct must mirror (host only)
extern "C" int grx_sim_sensors_layout(long long* out, int cap) {
  const grx_sim_sensors* z = nullptr;
#define OFF(f) (long long)((const char*)&z->f - (const char*)z)
  const long long v[] = {(long long)sizeof(grx_sim_sensors), OFF(spec), OFF(cutoff), OFF(nsensor), OFF(ndata), OFF(data)};
#undef OFF
  const int n = (int)(sizeof(v) / sizeof(v[0]));
  if (out) for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
  return n;
}
