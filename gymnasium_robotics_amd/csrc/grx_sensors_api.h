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
    const bool site_only = type == GRX_SNS_VELOCIMETER || type == GRX_SNS_GYRO || type == GRX_SNS_ACCELEROMETER;
    const bool ok = joint ? objtype == GRX_SNS_OBJ_JOINT : act ? objtype == GRX_SNS_OBJ_ACTUATOR : site_only ? objtype == GRX_SNS_OBJ_SITE : (objtype == GRX_SNS_OBJ_SITE || objtype == GRX_SNS_OBJ_XBODY);
    if (!ok) return fail(who + ": type " + std::to_string(type) + " does not read an object of type " + std::to_string(objtype) + " (joint types read joints, actuator types actuators, velocimeter / gyro / accelerometer sites, the frame types sites or xbodies)");
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

// The stepper with the fifth block.  params, dyn, con and frc may be null and mean what they mean to grx_sim_step_frc; a block without data or without sensors launches what
// that call launches for the other arguments.
extern "C" int grx_sim_step_sns(const grx_model* m, const grx_sim_params* p, const grx_sim_buffers* buf, const grx_sim_dynamics* dyn, const grx_sim_contacts* con, const grx_sim_applied* frc, const grx_sim_sensors* sns,
                                int n_worlds, int nstep, int forward_only, void* stream) {
  if (!sns) return fail("grx_sim_step_sns: null sensor block (grx_sim_step_frc is the call without one)");
  const GrxModel* desc;
  if (grx_sim_params_desc(m, p, n_worlds, &desc)) return -1;
  GrxSimStepArgs s = {m, buf, dyn, n_worlds, nstep, forward_only, stream, desc, con, frc};
  if (!sns->data || sns->nsensor == 0) return grx_sim_step_impl(s);
  if (sns->nsensor < 0 || sns->ndata < 1) return fail("grx_sim_step_sns: nsensor < 0 or ndata < 1 with a data buffer set");
  if (!sns->spec || !sns->cutoff) return fail("grx_sim_step_sns: null spec / cutoff table (host arrays [nsensor, 4] and [nsensor])");
  if (!m) return fail("grx_sim_step: null model");
  GrxSimSensors d; memset(&d, 0, sizeof(d));
  d.nsensor = sns->nsensor; d.ndata = sns->ndata; d.data = sns->data;
  if (grx_sensor_table(m, sns, &d.spec, &d.cutoff)) return -1;
  s.sns = &d;
  return grx_sim_step_impl(s);
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
