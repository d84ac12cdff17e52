// kb_load.cpp — kb_session_load (host session, every upload through one pinned area, proportion's water-fill as a launch, the load's one
// synchronisation) and kb_session_reset.  Split out of kb_engine.cpp in round 6 without a change of behaviour (kb_engine_int.hpp has the map).
// The load is a sequence of steps over one LoadCtx, in the order of its validations and stream operations: node state, the commit window and the
// 32-bit key range, node classes and key masks, task arrays (with backfill's t_fit), compat table, host ports, affinity table, inter-pod tables,
// jobs / queues / deserved, pristine copies, the closing reduction.  Every KbDev view is bound on the line of its upload (Uploader hands back the device pointer; an absent
// table stays the nullptr of `dev = KbDev{}`), and the buffers an action changes are listed ONCE, in for_each_live: the load's pristine copies
// and kb_session_reset's restore both walk that list.
#include "kb_engine_int.hpp"

#include <tuple>

// proportion's OnSessionOpen water-fill as a launch (kb_waterfill.hip; default since its first device run, round 4; KB_DEVICE_WATERFILL=0: the host loop): the queues' requests, weights and the
// session's total go up, `deserved` comes back for the host's order machine (Overused, the queue order) and stays on the device for
// k_finalize_queues.  build_host_session left hs.deserved at zero.
// Queued on the engine's stream, nothing waited for: the launch leaves `deserved` where k_finalize_queues reads it (b_deserved / b_desmask,
// in their [R][Q] layout) and the queue records and flags travel back into the load's pinned area; waterfill_collect reads them behind
// the synchronisation that ends the load (run_finalize's).
struct WaterfillInFlight { WfQueue *qs = nullptr; WfState *st = nullptr; };
static WaterfillInFlight device_waterfill_queue(kb_engine *e) {
  HostSession &hs = e->hs;
  const uint32_t Q = hs.Q;
  const size_t nq = Q ? Q : 1;
  WaterfillInFlight w;
  w.qs = reinterpret_cast<WfQueue *>(e->load_arena.take(sizeof(WfQueue) * nq));
  w.st = reinterpret_cast<WfState *>(e->load_arena.take(sizeof(WfState)));
  for (size_t q = 0; q < nq; q++) new (&w.qs[q]) WfQueue();
  new (w.st) WfState();
  for (uint32_t q = 0; q < Q; q++) {
    w.qs[q].request = hs.queue_request[q];
    w.qs[q].weight = hs.queue_weight[q];
    w.qs[q].has_attr = hs.queue_has_attr[q];
    w.qs[q].meet = 0;
    w.qs[q].active = 0;
  }
  WfState &st = *w.st;
  st.remaining = hs.total;
  st.total_weight = 0; st.stop = 0; st.share_at_open = 1; st.underflow = 0; st.passes = 0;
  DevBuf &b_q = e->b_wf_queues, &b_st = e->b_wf_state;   // kept between loads (the Go action loads a session every cycle): grown, never shrunk
  b_q.alloc(sizeof(WfQueue) * nq);
  b_st.alloc(sizeof(WfState));
  e->b_deserved.alloc(sizeof(double) * (size_t)hs.R * nq);
  e->b_desmask.alloc(sizeof(uint32_t) * nq);
  HIP_OK(hipMemcpyAsync(b_q.p, w.qs, sizeof(WfQueue) * nq, hipMemcpyHostToDevice, e->stream));
  HIP_OK(hipMemcpyAsync(b_st.p, w.st, sizeof(WfState), hipMemcpyHostToDevice, e->stream));
  kb_launch_waterfill(b_q.as<WfQueue>(), Q, b_st.as<WfState>(), hs.R, e->b_deserved.as<double>(), e->b_desmask.as<uint32_t>(), e->stream);
  HIP_OK(hipMemcpyAsync(w.qs, b_q.p, sizeof(WfQueue) * nq, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipMemcpyAsync(w.st, b_st.p, sizeof(WfState), hipMemcpyDeviceToHost, e->stream));
  return w;
}
static void waterfill_collect(kb_engine *e, const WaterfillInFlight &w) {
  HostSession &hs = e->hs;
  HIP_OK(hipGetLastError());
  if (w.st->underflow) throw EngineError(KB_E_UNSUPPORTED, "proportion water-filling underflow (the reference would panic in Resource.Sub)");
  for (uint32_t q = 0; q < hs.Q; q++) hs.deserved[q] = w.qs[q].deserved;
  hs.queue_share_at_open = w.st->share_at_open ? 1 : 0;
  e->waterfill_passes = w.st->passes;
}

// ---- the device state an action changes, listed ONCE: each live buffer and whether the loaded session has it; e->p_live[i] is the copy of entry i
//      as of the load.  f(live, pristine) for every entry present, in list order.  A new live buffer is ONE line here (b_tbind and b_jallocated
//      are cleared, not restored: clear_action_marks)
template <typename F> static void for_each_live(kb_engine *e, F f) {
  const bool ports = e->dev.ports != nullptr, ports_x = e->dev.ports_x != nullptr, interpod = e->hs.has_interpod;
  const struct { DevBuf &live; bool present; } list[] = {
      {e->b_idle, true}, {e->b_rel, true}, {e->b_nzc, true}, {e->b_nzm, true}, {e->b_podcnt, true}, {e->b_tstatus, true}, {e->b_tnode, true},
      {e->b_ports, ports}, {e->b_ports_x, ports_x}, {e->b_tcounted, true},
      {e->b_nmask, true},   // the evict actions rewrite the key masks of the nodes they touch (upload_live_nodes)
      {e->b_ip_ccnt, interpod}, {e->b_ip_ctot, interpod}, {e->b_ip_punb, interpod}, {e->b_ip_z, interpod},
  };
  if (!e->p_live) e->p_live.reset(new DevBuf[std::size(list)]);
  for (size_t i = 0; i < std::size(list); i++)
    if (list[i].present) f(list[i].live, e->p_live[i]);
}
// nothing is bound and no job has an Allocate yet: t_bind KB_NONE everywhere, j_allocated 0, set on the device
static void clear_action_marks(kb_engine *e) {
  static_assert(KB_NONE == 0xFFFFFFFFu, "t_bind is cleared with a byte pattern");
  HIP_OK(hipMemsetAsync(e->b_tbind.p, 0xFF, e->b_tbind.bytes, e->stream));
  HIP_OK(hipMemsetAsync(e->b_jallocated.p, 0, e->b_jallocated.bytes, e->stream));
}

// ---- kb_session_load's steps.  They throw EngineError like the load itself; e->async_pending is set before the first of them queues a copy.
struct LoadCtx {
  kb_engine *e; const kb_snapshot *sn; Uploader up; uint32_t NP;
  // build_host_session's.  Owned here, not by a step: t_active goes up through copy_persistent, which from 8 MiB on copies straight from the vector,
  // so it must be alive at the load's one synchronisation (run_finalize's)
  std::vector<uint32_t> t_active, nmask;
};
static void upload_node_state(LoadCtx &c) {
  kb_engine *e = c.e; const kb_snapshot *sn = c.sn; KbDev &d = e->dev; Uploader &up = c.up;
  const uint32_t N = d.N, NP = c.NP;
  d.idle = up.padded(e->b_idle, sn->node_idle, d.R, N, NP);
  e->idle_below_eps = false;   // NodeInfo keeps Idle above -epsilon (every Sub is guarded by LessEqual); a snapshot may not
  for (uint32_t n = 0; n < N; n++)
    if (sn->node_idle[n] <= -kMinMilliCPU || sn->node_idle[(size_t)N + n] <= -kMinMemory) e->idle_below_eps = true;
  d.rel = up.padded(e->b_rel, sn->node_releasing, d.R, N, NP);
  d.nzc = up.padded(e->b_nzc, sn->node_nz_cpu, 1, N, NP);
  d.nzm = up.padded(e->b_nzm, sn->node_nz_mem, 1, N, NP);
  d.podcnt = up.padded(e->b_podcnt, sn->node_pod_cnt, 1, N, NP);
  d.acpu = up.padded(e->b_acpu, sn->node_alloc_cpu, 1, N, NP);
  d.amem = up.padded(e->b_amem, sn->node_alloc_mem, 1, N, NP);
  d.maxpods = up.padded(e->b_maxpods, sn->node_max_pods, 1, N, NP);
  // reciprocals of the allocatable quantities for the exact integer-division estimate (IEEE division, same on host and device)
  auto reciprocals = [&](DevBuf &b, const int64_t *alloc) {
    double *inv = up.stage<double>(b, NP);
    for (uint32_t n = 0; n < N; n++) inv[n] = 1.0 / (double)alloc[n];
    std::fill(inv + N, inv + NP, 0.0);
    return up.commit(inv);
  };
  d.inv_acpu = reciprocals(e->b_invac, sn->node_alloc_cpu);
  d.inv_amem = reciprocals(e->b_invam, sn->node_alloc_mem);
}
// The commit kernel keeps the window in LDS (160 KiB per workgroup on gfx950): one dirty slot per row (one thread of the 256-thread workgroup
// evaluates one slot), the row descriptors, and per distinct shape its candidate list.  Prefer the largest window that still admits 64 shapes.
static std::pair<uint32_t, uint32_t> plan_commit_window(uint32_t window, uint32_t NP, int R) {   // -> (eff_window, shape_cap)
  const uint32_t budget = 160u * 1024u;
  const uint32_t W = std::min<uint32_t>(window, KB_K5_MAX_ROWS);
  uint32_t best_w = 0, best_s = 0;
  for (uint32_t w = W; w >= 1; w = (w > 32 ? ((w - 1) / 32) * 32 : w - 1)) {
    uint32_t sc = std::min<uint32_t>(KB_K5_MAX_SHAPES, w);
    while (sc > 0 && kb_commit_smem_bytes(w, sc, NP, R) > budget) sc--;
    if (sc >= std::min<uint32_t>(64, w)) { best_w = w; best_s = sc; break; }
    if (sc > best_s) { best_w = w; best_s = sc; }
    if (w == 1) break;
  }
  if (best_w == 0 || best_s == 0) throw EngineError(KB_E_UNSUPPORTED, "too many nodes / resource dimensions for the commit kernel's LDS tables");
  return {best_w, best_s};
}
// 32-bit keys: (score + 1) << node_bits | inverted node index
static void check_key_range(const Policy &pol, uint32_t NP) {
  if (((unsigned long long)(max_score(pol, false) + 2) << kb_node_bits(NP)) > (1ull << 32))
    throw EngineError(KB_E_UNSUPPORTED, "score range x node count exceeds the commit kernel's 32-bit keys");
}
static void upload_node_classes(LoadCtx &c) {
  KbDev &d = c.e->dev;
  d.ncls = c.up.padded<uint32_t>(c.e->b_ncls, c.sn->node_class, c.sn->node_class ? 1 : 0, d.N, c.NP);   // no classes: every node is of class 0
  d.nmask = c.up.copy(c.e->b_nmask, c.nmask.data(), c.NP);
}
static void upload_task_arrays(LoadCtx &c) {
  kb_engine *e = c.e; const kb_snapshot *sn = c.sn; KbDev &d = e->dev; Uploader &up = c.up; HostSession &hs = e->hs;
  const uint32_t T = d.T, J = d.J;
  const size_t RT = (size_t)d.R * T;
  d.t_init = up.copy_persistent(e->b_tinit, hs.t_init.data(), RT);
  e->t_fit = d.t_init;
  // the backfill view of t_init: cpu / memory of a BestEffort task are its Resreq (scalar rows are never compared for
  // them: every InitResreq scalar is at or below the epsilon, resource_info.go:283-287)
  bool differs = false;
  for (uint32_t t = 0; t < T && !differs; t++)
    differs = hs.t_init_empty[t] && (hs.t_res[t] != hs.t_init[t] || hs.t_res[(size_t)T + t] != hs.t_init[(size_t)T + t]);
  if (differs) {
    std::vector<double> fit(hs.t_init);
    for (uint32_t t = 0; t < T; t++)
      if (hs.t_init_empty[t]) { fit[t] = hs.t_res[t]; fit[(size_t)T + t] = hs.t_res[(size_t)T + t]; }
    e->t_fit = up.copy(e->b_tfit, fit.data(), RT);
  }
  d.t_res = up.copy_persistent(e->b_tres, hs.t_res.data(), RT);
  d.t_nzc = up.copy_persistent(e->b_tnzc, sn->task_nz_cpu, T);
  d.t_nzm = up.copy_persistent(e->b_tnzm, sn->task_nz_mem, T);
  d.t_cls = up.copy_persistent(e->b_tcls, hs.t_cls.data(), T);
  d.t_active = up.copy_persistent(e->b_tactive, c.t_active.data(), T);
  d.t_resmask = up.copy_persistent(e->b_tresmask, hs.t_resmask.data(), T);
  d.t_job = up.copy_persistent(e->b_tjob, hs.t_job.data(), T);
  d.t_status = up.copy_persistent(e->b_tstatus, hs.t_status.data(), T);
  d.t_node = up.copy_persistent(e->b_tnode, hs.t_node.data(), T);
  uint8_t *counted = up.stage<uint8_t>(e->b_tcounted, T);
  for (uint32_t t = 0; t < T; t++) counted[t] = is_allocated_status(hs.t_status[t]) ? 1 : 0;   // drf.go:71-77
  d.t_counted = up.commit(counted);
  e->b_tbind.alloc(sizeof(uint32_t) * (T ? T : 1));
  e->b_jallocated.alloc(J ? J : 1);
  d.t_bind = e->b_tbind.as<uint32_t>(); d.j_allocated = e->b_jallocated.as<uint8_t>();
  clear_action_marks(e);
}
// every task's and node's class lies inside the class tables (called in front of each table that is indexed by them)
static void check_class_ranges(const LoadCtx &c) {
  const kb_snapshot *sn = c.sn;
  for (uint32_t t = 0; t < c.e->hs.T; t++)
    if (c.e->hs.t_cls[t] >= sn->n_task_classes) throw EngineError(KB_E_INVALID, "task class out of range");
  for (uint32_t n = 0; n < c.e->hs.N; n++)
    if ((sn->node_class ? sn->node_class[n] : 0u) >= sn->n_node_classes) throw EngineError(KB_E_INVALID, "node class out of range");
}
static void upload_compat_table(LoadCtx &c) {
  kb_engine *e = c.e; const kb_snapshot *sn = c.sn; KbDev &d = e->dev;
  d.n_nc = sn->n_node_classes ? sn->n_node_classes : 1;
  if (!sn->class_compat) return;
  check_class_ranges(c);
  d.compat = c.up.copy(e->b_compat, sn->class_compat, ((size_t)sn->n_task_classes * sn->n_node_classes + 7) / 8);
  if (sn->n_node_classes > 256) return;
  std::vector<uint32_t> rows((size_t)sn->n_task_classes * 8, 0u);   // word-aligned rows for the commit kernel (one 32-byte fetch per task class)
  for (uint32_t tc = 0; tc < sn->n_task_classes; tc++)
    for (uint32_t nc = 0; nc < sn->n_node_classes; nc++) {
      size_t bit = (size_t)tc * sn->n_node_classes + nc;
      if ((sn->class_compat[bit >> 3] >> (bit & 7)) & 1) rows[(size_t)tc * 8 + (nc >> 5)] |= 1u << (nc & 31);
    }
  d.crows = c.up.copy(e->b_crows, rows.data(), rows.size());
}
static void upload_host_ports(LoadCtx &c) {
  kb_engine *e = c.e; const kb_snapshot *sn = c.sn; KbDev &d = e->dev; Uploader &up = c.up; HostSession &hs = e->hs;
  if (!(sn->node_ports || sn->task_port_want || sn->task_port_conflict)) return;
  const uint32_t N = d.N, NP = c.NP, T = d.T;
  const size_t Wh = mask_words(64ull * sn->port_words);   // 64-bit words per mask; word 0 here, the others below
  std::vector<unsigned long long> np_(NP, 0ull), tw(T ? T : 1, 0ull), tc(T ? T : 1, 0ull);
  bool any = false;
  for (uint32_t n = 0; n < N && sn->node_ports; n++) { np_[n] = sn->node_ports[(size_t)n * Wh]; any = any || np_[n]; }
  for (uint32_t t = 0; t < T; t++) {
    if (sn->task_port_want) tw[t] = sn->task_port_want[(size_t)t * Wh];
    if (sn->task_port_conflict) tc[t] = sn->task_port_conflict[(size_t)t * Wh];
    if ((tw[t] & ~tc[t]) != 0) throw EngineError(KB_E_INVALID, "a pod's host ports must conflict with themselves (want is not a subset of conflict)");
    any = any || tw[t] || tc[t];
  }
  auto upload_word0 = [&] {
    d.ports = up.copy(e->b_ports, np_.data(), NP);
    d.t_want = up.copy(e->b_twant, tw.data(), tw.size());
    d.t_conf = up.copy(e->b_tconf, tc.data(), tc.size());
  };
  if (any) upload_word0();
  if (!hs.port_xw) return;
  // some pod reaches beyond word 0 (kb_host.hpp: t_wide): the words behind it, nodes word-major ([port_xw][NP]: K1 reads runs of nodes)
  const uint32_t X = hs.port_xw;
  std::vector<unsigned long long> nx((size_t)X * NP, 0ull);
  for (uint32_t n = 0; n < N && sn->node_ports; n++)
    for (uint32_t w = 0; w < X; w++) nx[(size_t)w * NP + n] = sn->node_ports[(size_t)n * Wh + 1 + w];
  d.ports_x = up.copy(e->b_ports_x, nx.data(), nx.size());
  d.t_want_x = up.copy_persistent(e->b_twant_x, hs.t_want_x.data(), hs.t_want_x.size());
  d.t_conf_x = up.copy_persistent(e->b_tconf_x, hs.t_conf_x.data(), hs.t_conf_x.size());
  d.port_xw = X;
  if (!d.ports) upload_word0();   // word 0 empty everywhere: the kernels still take the host-port path by d.ports
}
static void upload_affinity_table(LoadCtx &c) {
  kb_engine *e = c.e; const kb_snapshot *sn = c.sn; KbDev &d = e->dev; HostSession &hs = e->hs;
  hs.cls_has_aff.clear();
  d.wNA = e->pol.wNA;
  if (!(sn->class_affinity && sn->n_task_classes && sn->n_node_classes)) return;
  check_class_ranges(c);
  std::vector<uint8_t> has(sn->n_task_classes, 0);
  bool any = false;
  for (uint32_t tc = 0; tc < sn->n_task_classes; tc++)
    for (uint32_t nc = 0; nc < sn->n_node_classes; nc++) {
      const int32_t cnt = sn->class_affinity[(size_t)tc * sn->n_node_classes + nc];
      if (cnt < 0 || cnt > 100000) throw EngineError(KB_E_UNSUPPORTED, "node-affinity count outside 0..100000");
      if (cnt) { has[tc] = 1; any = true; }
    }
  if (!any || e->pol.wNA == 0) return;
  if (e->pol.wNA < 0 || max_score(e->pol, false) > 65535)
    throw EngineError(KB_E_UNSUPPORTED, "nodeorder weights exceed the 16-bit score range");
  hs.has_affinity = true;
  hs.cls_has_aff = has;
  d.aff = c.up.copy(e->b_aff, sn->class_affinity, (size_t)sn->n_task_classes * sn->n_node_classes);
  d.aff_cls = c.up.copy(e->b_affcls, has.data(), has.size());
}
static void upload_interpod_tables(LoadCtx &c) {
  kb_engine *e = c.e; KbDev &d = e->dev; Uploader &up = c.up; HostSession &hs = e->hs;
  const kb_interpod *ip = c.sn->interpod;
  d.ip_Wc = d.ip_Wp = 1; d.wPA = e->pol.wPA;
  if (!ip) return;
  const uint32_t N = d.N, T = d.T, C = ip->n_counters, P = ip->n_classes, D = ip->n_domains;
  const uint32_t Wc = hs.ip_Wc, Wp = hs.ip_Wp;
  // [rows][N] -> [max(rows, 1)][NP], the pad (and the row of a table without rows) KB_NONE / 0
  d.ip_ctr_dom = up.padded<uint32_t>(e->b_ip_cdom, ip->ctr_dom, C, N, c.NP, KB_NONE);
  d.ip_cls_dom = up.padded<uint32_t>(e->b_ip_pdom, ip->cls_dom, P, N, c.NP, KB_NONE);
  d.ip_cls_bound = up.padded<int32_t>(e->b_ip_pbound, ip->cls_bound, P, N, c.NP, 0);
  d.ip_cls_unbound = up.padded<int32_t>(e->b_ip_punb, ip->cls_unbound, P, N, c.NP, 0);
  std::vector<int32_t> cc((size_t)std::max(C, 1u) * D, 0), ct(std::max(C, 1u), 0);
  if (C) { std::memcpy(cc.data(), ip->ctr_count, sizeof(int32_t) * (size_t)C * D); std::memcpy(ct.data(), ip->ctr_total, sizeof(int32_t) * C); }
  d.ip_ctr_count = up.copy(e->b_ip_ccnt, cc.data(), cc.size());
  d.ip_ctr_total = up.copy(e->b_ip_ctot, ct.data(), ct.size());
  d.t_ip_inc = up.copy_persistent(e->b_ip_tinc, ip->task_inc, (size_t)T * Wc);
  d.t_ip_forbid = up.copy_persistent(e->b_ip_tforbid, ip->task_forbid, (size_t)T * Wc);
  d.t_ip_checks = up.copy(e->b_ip_tchk, hs.t_ip_checks.data(), T);
  d.t_ip_req = up.copy(e->b_ip_treq, ip->task_require, T);
  d.t_ip_self = up.copy(e->b_ip_tself, ip->task_self, T);
  d.t_ip_subject = up.copy(e->b_ip_tsubj, hs.t_ip_subject.data(), T);
  d.t_ip_cls_inc = up.copy_persistent(e->b_ip_tcinc, ip->task_cls_inc, (size_t)T * Wp);
  d.t_ip_sig = up.copy(e->b_ip_tsig, ip->task_sig, T);
  std::vector<int32_t> sw((size_t)std::max(ip->n_sigs, 1u) * std::max(P, 1u), 0);
  if (ip->n_sigs && P) std::memcpy(sw.data(), ip->sig_weight, sizeof(int32_t) * (size_t)ip->n_sigs * P);
  d.ip_sig_w = up.copy(e->b_ip_sigw, sw.data(), sw.size());
  const uint32_t z0 = ip->first_unbound_node;
  d.ip_z = up.copy(e->b_ip_z, &z0, 1);
  d.ip_C = C; d.ip_D = D; d.ip_P = P; d.ip_Wc = Wc; d.ip_Wp = Wp;
}
// jobs, queues, `deserved`, the probe's mapped rows, and everything the engine remembers per session
static void upload_jobs_and_queues(LoadCtx &c) {
  kb_engine *e = c.e; KbDev &d = e->dev; Uploader &up = c.up; HostSession &hs = e->hs;
  const int R = d.R;
  const uint32_t J = d.J, Q = d.Q;
  e->h_probe_alive.resize(std::max<uint32_t>(hs.n_feas_shapes, 1u));
  e->h_probe_rows.resize(std::max<uint32_t>(hs.n_feas_shapes, 1u));
  HIP_OK(hipHostGetDevicePointer((void **)&e->d_probe_alive, e->h_probe_alive.data(), 0));
  HIP_OK(hipHostGetDevicePointer((void **)&e->d_probe_rows, e->h_probe_rows.data(), 0));
  up.copy(e->b_jbegin, hs.job_begin.data(), J + 1);
  up.copy(e->b_jmin, hs.job_min.data(), J);
  up.copy(e->b_jqueue, hs.job_queue.data(), J);
  up.copy(e->b_total, hs.total.v, KB_MAX_RES);
  e->total_mask = hs.total.mask;
  if (!hs.waterfill_on_device) {   // the host loop of kb_session.cpp filled hs.deserved (the launch writes b_deserved / b_desmask itself)
    double *des = up.stage<double>(e->b_deserved, (size_t)R * (Q ? Q : 1));
    std::fill(des, des + (size_t)R * (Q ? Q : 1), 0.0);
    for (uint32_t q = 0; q < Q; q++)
      for (int dd = 0; dd < R; dd++) des[(size_t)dd * Q + q] = hs.deserved[q].get(dd);
    up.commit(des);
    uint32_t *desmask = up.stage<uint32_t>(e->b_desmask, Q ? Q : 1);
    desmask[0] = 0;
    for (uint32_t q = 0; q < Q; q++) desmask[q] = hs.deserved[q].mask;
    up.commit(desmask);
  }
  hs.job_alloc.assign((size_t)J * R, 0.0);
  hs.job_share.assign(J, 0.0);
  hs.queue_alloc.assign((size_t)Q * R, 0.0);
  hs.queue_share.assign(Q, 0.0);
  hs.job_ready.assign(J, 0);
  e->b_jalloc.alloc(sizeof(double) * (size_t)(J ? J : 1) * R);
  e->b_jshare.alloc(sizeof(double) * (J ? J : 1));
  e->b_qalloc.alloc(sizeof(double) * (size_t)(Q ? Q : 1) * R);
  e->b_qshare.alloc(sizeof(double) * (Q ? Q : 1));
  e->b_jready.alloc(sizeof(int) * (J ? J : 1));
  d.wL = e->pol.wL; d.wM = e->pol.wM; d.wB = e->pol.wB;
  d.pred_enabled = e->pol.pred_enabled ? 1 : 0;
  d.score_enabled = e->pol.nodeorder_enabled ? 1 : 0;
  d.whole = hs.whole ? 1u : 0u;
  e->win_cap = 0; e->mat_cap = 0; e->keys_cap = 0;
  e->mat2_cap = 0; e->stale_cap = 0;   // the second stream's matrix rows are [rows][NP] too: a session with more nodes needs them again
  e->xs_cap = 0;   // kb_eval_matrix's per-shape rows are [shapes][NP] as well (found by tests/test_gpu_reload.py: fewer shapes over more nodes overran them)
  e->stats = kb_stats{};
  e->dirty_share = 0.0;
  e->commit_kernel = e->commit_pin >= 0 ? e->commit_pin : (int)KB_COMMIT_SELECT;
  e->round_no = 0;
}
static void take_pristine_copies(kb_engine *e) {
  for_each_live(e, [&](DevBuf &live, DevBuf &pristine) { pristine.copy_of(live, e->stream); });
}
// initial drf / proportion / gang aggregates come from the device reduction (K2+K4): the load's synchronisation; the water-fill's answer (deserved,
// "did a pass run") is read behind it, in front of the host-side post-processing of the shares, which wants to know whether updateShare ran at open
static void reduce_and_finish(kb_engine *e, const WaterfillInFlight &wf) {
  HostSession &hs = e->hs;
  run_finalize(e, [&]() {
    if (hs.waterfill_on_device) waterfill_collect(e, wf);
    hs.queue_share_live.assign(hs.Q ? hs.Q : 1, hs.queue_share_at_open);
  });
  e->fin0.job_alloc = hs.job_alloc; e->fin0.job_share = hs.job_share; e->fin0.queue_alloc = hs.queue_alloc; e->fin0.queue_share = hs.queue_share;
  e->fin0.job_ready = hs.job_ready; e->fin0.t_status = hs.t_status; e->fin0.t_node = hs.t_node; e->fin0.valid = true;
  e->stats.reduce_ms = 0;
  e->loaded = true;
  e->tainted = false;
}

extern "C" {

int kb_session_load(kb_engine *e, const kb_snapshot *sn) {
  if (!e) return KB_E_INVALID;
  return guarded(e, [&]() {
    if (!sn) throw EngineError(KB_E_INVALID, "snapshot is NULL");
    if (sn->version != KB_ABI_VERSION) throw EngineError(KB_E_INVALID, "snapshot ABI version mismatch");
    if (sn->n_res < 2 || sn->n_res > KB_MAX_RES) throw EngineError(KB_E_INVALID, "n_res out of range");
    quiesce(e);
    e->loaded = false;
    e->fin0.valid = false;
    e->stale_checked = false; e->pristine = true; e->load_clean = false;
    mg_reset(e->mg);   // (its device buffers are grow-only like every other one: no hipFree / hipMalloc per cycle)
    HostSession &hs = e->hs;
    const uint32_t NP = ((sn->n_nodes + KB_NODE_PAD - 1) / KB_NODE_PAD) * KB_NODE_PAD + (sn->n_nodes == 0 ? KB_NODE_PAD : 0);
    LoadCtx c{e, sn, Uploader(e->load_arena, e->stream), NP, {}, {}};
    hs.waterfill_on_device = e->device_waterfill && e->pol.has_proportion;
    PhaseTrace trace("kb_session_load: ", 28);
    build_host_session(sn, e->pol, NP, hs, c.t_active, c.nmask);   // kb_session.cpp: validation, shapes, plugin OnSessionOpen state
    trace.mark("build_host_session");
    e->evictions.clear();
    // ---- device upload: sources through the pinned area, copies asynchronous on the engine's stream, ONE synchronisation: reduce_and_finish's
    e->load_arena.reset();
    e->async_pending = true;   // from here on copies out of (and the water-fill's answers into) the pinned area are queued: a validation that throws below
                               // leaves them in flight, and the next load's quiesce() must wait for them before the area is handed out again
    // proportion's water-fill first: it needs the host session only, and its (tiny, serial) launch runs while the host assembles the rest
    const WaterfillInFlight wf_flight = hs.waterfill_on_device ? device_waterfill_queue(e) : WaterfillInFlight{};
    KbDev &d = e->dev = KbDev{};   // an absent table is the nullptr (the zero count) of this line; the steps bind what they upload
    d.R = hs.R; d.N = hs.N; d.NP = NP; d.T = hs.T; d.J = hs.J; d.Q = hs.Q;
    upload_node_state(c);
    std::tie(e->eff_window, e->shape_cap) = plan_commit_window(e->window, NP, hs.R);
    check_key_range(e->pol, NP);
    trace.mark("node arrays, window");
    upload_node_classes(c);
    upload_task_arrays(c);
    trace.mark("task arrays");
    upload_compat_table(c);
    upload_host_ports(c);
    upload_affinity_table(c);
    upload_interpod_tables(c);
    trace.mark("classes, ports, inter-pod");
    upload_jobs_and_queues(c);
    trace.mark("jobs, queues, deserved");
    take_pristine_copies(e);
    trace.mark("pristine copies (queued)");
    reduce_and_finish(e, wf_flight);
    trace.mark("aggregates (device reduction, the load's one synchronisation)");
  });
}

int kb_session_reset(kb_engine *e) {
  if (!e) return KB_E_INVALID;
  return guarded(e, [&]() {
    if (!e->loaded) throw EngineError(KB_E_STATE, "no session loaded");
    const double t_reset0 = now_ms();
    e->tainted = false;
    e->pristine = true;
    e->stale_checked = e->load_clean;
    for_each_live(e, [&](DevBuf &live, DevBuf &pristine) { HIP_OK(hipMemcpyAsync(live.p, pristine.p, pristine.bytes, hipMemcpyDeviceToDevice, e->stream)); });
    clear_action_marks(e);
    mg_reset(e->mg);   // (its device buffers are grow-only like every other one: no hipFree / hipMalloc per cycle)
    std::fill(e->hs.queue_share_live.begin(), e->hs.queue_share_live.end(), e->hs.queue_share_at_open);
    e->evictions.clear();
    e->hs.t_off_node.clear();
    // The restored state is bit for bit the one kb_session_load reduced (the pristine copies were taken in front of that reduction,
    // which flips no status: no job has an Allocate yet): its results come back from the host copies made then.  The device-side result
    // buffers keep the previous reduction's values; nothing reads them before the next reduction rewrites them.
    if (e->fin0.valid) {
      e->async_pending = true;   // stream-ordered with everything run_allocate / run_backfill launch; quiesce() for the rest
      HostSession &hs = e->hs;
      hs.job_alloc = e->fin0.job_alloc; hs.job_share = e->fin0.job_share; hs.queue_alloc = e->fin0.queue_alloc; hs.queue_share = e->fin0.queue_share;
      hs.job_ready = e->fin0.job_ready; hs.t_status = e->fin0.t_status; hs.t_node = e->fin0.t_node;
    } else {
      double keep = e->stats.reduce_ms;
      run_finalize(e);
      e->stats.reduce_ms = keep;
    }
    e->tl_reset += now_ms() - t_reset0;
  });
}

}  // extern "C"
