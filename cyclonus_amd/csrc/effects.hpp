// effects.hpp — which target decides: the host side of cyc_probe_target_effects (kernels: dev_effects.hpp).
// Part of engine.hip's single translation unit, included after enqueue.hpp.
#pragma once

// The batch buffers' cap (dev_effects.hpp).  CYC_EFFECTS_SCRATCH_KB lowers or raises it for one process: a
// development aid like CYC_TRACE_PREPARE, which lets a small problem go through several batches and windows.
static uint64_t effects_scratch_cap() {
  const char* e = getenv("CYC_EFFECTS_SCRATCH_KB");
  if (e && *e) {
    const long long kb = atoll(e);
    if (kb > 0) return uint64_t(kb) << 10;
  }
  return EFF_SCRATCH_CAP;
}

namespace {
struct EffClass {  // target pods of the rows with one set of applying targets (ingress: and one descriptor per slot)
  uint32_t list, row, pods;
};
struct EffBatch {
  std::vector<uint32_t> tl;   // its targets, ascending
  std::vector<uint32_t> cls;  // its classes
  uint32_t WA = 0;            // words per window
};
std::string bytes_of(const void* p, size_t n) { return std::string(static_cast<const char*>(p), n); }
}  // namespace

// The call's body (cyc_probe_target_effects checked the arguments and zeroed the outputs; rows, T > 0).
static int target_effects(cyc_ctx* c, int d, int64_t row_lo, int64_t row_hi, int64_t k_lo, int64_t k_hi, int64_t* effects,
                          int64_t* applies) {
  const Problem& pb = c->pb;
  const Prepared& pr = c->prep;
  hipStream_t st = c->stream;
  const uint32_t P = pb.P, K = pb.K, W = pb.W, T = uint32_t(pb.tgt[d].size()), nk = uint32_t(k_hi - k_lo);
  const uint32_t D = uint32_t(std::max<size_t>(pb.descs.size(), 1)), M = uint32_t(pb.pms.size());
  const uint64_t cap = effects_scratch_cap();
  uint64_t fixed = 0, peak = 0;  // scratch: tables alive for the whole call; with the batch buffers
  auto held = [&](const DevBuf& b) { fixed += b.bytes; };
  // CYC_TRACE_PREPARE=1: the call's host phases on stderr, and (synchronising after each) its kernels' times
  PhaseClock clk("effects");
  double k_ms[4] = {0, 0, 0, 0};  // allow rows, population counts, sole sweep, whatever else the stream held
  auto kernel_done = [&](int which) {
    if (!clk.on) return;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipStreamSynchronize(st));  // (the launches before it were timed by the previous call)
    k_ms[which] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };

  // ---- the port table (k_portok), the call's own copy
  DevBuf portok;
  portok.alloc(std::max<uint64_t>(uint64_t(M) * D, 16));
  held(portok);
  const PortArgs pa{grid1(uint64_t(M) * D, 256), M, D, pr.pms.as<DPortM>(), pr.pents.as<DPortEntry>(), pr.descs.as<DDesc>(),
                    portok.as<uint8_t>()};
  if (pa.nb) k_portok<<<pa.nb, 256, 0, st>>>(pa);
  HIPCHK(hipGetLastError());

  EffTables x{};
  x.P = P, x.K = K, x.W = W, x.D = D;
  x.pod_ns = pr.pod_ns.as<uint32_t>(), x.pod_ls = pr.pod_ls.as<uint32_t>(), x.pod_nsls = pr.pod_nsls.as<uint32_t>();
  x.pod_ip = pr.pod_ip.as<DIP>();
  x.sel_off = pr.sel_off.as<uint32_t>(), x.req_vals = pr.req_vals.as<uint32_t>(), x.reqs = pr.reqs.as<DReq>();
  x.ls_off = pr.ls_off.as<uint32_t>(), x.ls_key = pr.ls_key.as<uint32_t>(), x.ls_val = pr.ls_val.as<uint32_t>();
  x.peers = pr.peers.as<DPeer>(), x.ipbs = pr.ipbs.as<DIPBlock>(), x.cidrs = pr.cidrs.as<DCidr>();
  x.ipb_ex = pr.ipb_ex.as<uint32_t>();
  x.tgt = pr.dir[d].tgt.as<DTarget>(), x.tns_lo = pr.dir[d].tns_lo.as<uint32_t>(), x.tns_hi = pr.dir[d].tns_hi.as<uint32_t>();
  x.slot_desc = pr.slot_desc.as<int32_t>(), x.slot_status = pr.slot_status.as<uint8_t>();
  x.portok = portok.as<uint8_t>();

  // ---- TargetsApplyingToPod once per distinct (namespace, label set) of the rows' pods
  const uint32_t rows = uint32_t(row_hi - row_lo);
  std::vector<uint32_t> id_ns, id_ls, id_pods, pod_id(rows);
  {
    std::unordered_map<uint64_t, uint32_t> id_of;
    for (uint32_t r = 0; r < rows; r++) {
      const uint32_t q = uint32_t(row_lo) + r;
      auto it = id_of.emplace(uint64_t(pb.pod_ns[q]) << 32 | pb.pod_ls[q], uint32_t(id_ns.size()));
      if (it.second) id_ns.push_back(pb.pod_ns[q]), id_ls.push_back(pb.pod_ls[q]), id_pods.push_back(0);
      pod_id[r] = it.first->second;
      id_pods[pod_id[r]]++;
    }
  }
  const uint32_t n_id = uint32_t(id_ns.size());
  std::vector<uint32_t> cnt(n_id), off(n_id + 1, 0), list;
  {
    DevBuf d_ns, d_ls, d_cnt, d_off, d_list;
    upload(d_ns, id_ns);
    upload(d_ls, id_ls);
    d_cnt.alloc(uint64_t(n_id) * 4);
    EffMemberArgs ma{};
    ma.x = x, ma.n = n_id, ma.id_ns = d_ns.as<uint32_t>(), ma.id_ls = d_ls.as<uint32_t>(), ma.cnt = d_cnt.as<uint32_t>();
    k_eff_member<false><<<grid1(uint64_t(n_id) * 64, 256), 256, 0, st>>>(ma);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, uint64_t(n_id) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n_id; i++) {
      off[i] = uint32_t(tot);
      tot += cnt[i];
      if (tot > 0xFFFFFFFFull) throw Panic{CYC_ERR_OOM, "target effects: the rows' applying-target lists exceed 2^32 entries"};
    }
    off[n_id] = uint32_t(tot);
    list.resize(tot);
    if (tot) {
      upload(d_off, off);
      d_list.alloc(tot * 4);
      ma.off = d_off.as<uint32_t>(), ma.list = d_list.as<uint32_t>();
      k_eff_member<true><<<grid1(uint64_t(n_id) * 64, 256), 256, 0, st>>>(ma);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(list.data(), d_list.p, tot * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    peak = fixed + d_ns.bytes + d_ls.bytes + d_cnt.bytes + d_off.bytes + d_list.bytes;
  }
  clk.lap("membership");
  if (applies)
    for (uint32_t i = 0; i < n_id; i++)
      for (uint32_t e = off[i]; e < off[i + 1]; e++) applies[list[e]] += id_pods[i];
  c->effects.scratch = peak;
  if (!nk) return (int)CYC_OK;

  // ---- classes: (applying-target list, ingress: the slots' VALID descriptors) -> pods of the rows
  std::vector<uint32_t> lid_of(n_id), l_off, l_len;  // distinct lists: a representative's span in `list`
  {
    std::unordered_map<std::string, uint32_t> seen;
    for (uint32_t i = 0; i < n_id; i++) {
      auto it = seen.emplace(bytes_of(list.data() + off[i], size_t(cnt[i]) * 4), uint32_t(l_off.size()));
      if (it.second) l_off.push_back(off[i]), l_len.push_back(cnt[i]);
      lid_of[i] = it.first->second;
    }
  }
  std::vector<int32_t> row_desc;  // [distinct rows][nk]: the slot's descriptor when its job is VALID, else -1
  std::vector<EffClass> cls;
  {
    std::unordered_map<std::string, uint32_t> seen_row;
    std::unordered_map<uint64_t, uint32_t> seen_cls;
    std::vector<int32_t> rd(nk);
    for (uint32_t r = 0; r < rows; r++) {
      const uint32_t q = uint32_t(row_lo) + r, lid = lid_of[pod_id[r]];
      if (!l_len[lid]) continue;  // no target applies: no effect to count
      uint32_t rid = 0;
      if (d == 0) {
        for (uint32_t kk = 0; kk < nk; kk++) {
          const size_t at = size_t(q) * K + size_t(k_lo) + kk;
          rd[kk] = pb.slot_status[at] == CYC_JOB_VALID ? pb.slot_desc[at] : -1;
        }
        auto it = seen_row.emplace(bytes_of(rd.data(), size_t(nk) * 4), uint32_t(seen_row.size()));
        if (it.second) row_desc.insert(row_desc.end(), rd.begin(), rd.end());
        rid = it.first->second;
      }
      auto it = seen_cls.emplace(uint64_t(lid) << 32 | rid, uint32_t(cls.size()));
      if (it.second) cls.push_back(EffClass{lid, rid, 0});
      cls[it.first->second].pods++;
    }
  }
  if (cls.empty()) return (int)CYC_OK;
  // classes of one namespace side by side (their targets are one run of the primary-key order)
  std::sort(cls.begin(), cls.end(), [&](const EffClass& a, const EffClass& b) {
    const uint32_t fa = list[l_off[a.list]], fb = list[l_off[b.list]];
    return fa != fb ? fa < fb : a.list != b.list ? a.list < b.list : a.row < b.row;
  });

  clk.lap("classes");
  // ---- egress: the VALID pods of every (slot, descriptor) as bit rows, and their number per slot
  std::vector<int64_t> n_valid(nk, 0);
  DevBuf V;
  if (d == 1) {
    for (uint32_t q = 0; q < P; q++)
      for (uint32_t kk = 0; kk < nk; kk++) n_valid[kk] += pb.slot_status[size_t(q) * K + size_t(k_lo) + kk] == CYC_JOB_VALID;
    V.alloc(std::max<uint64_t>(uint64_t(nk) * D * W * 8, 16));
    held(V);
    EffValidArgs va{x, uint32_t(k_lo), nk, V.as<uint64_t>()};
    k_eff_valid<<<grid1(uint64_t(nk) * W * 64, 256), 256, 0, st>>>(va);
    HIPCHK(hipGetLastError());
  }

  // ---- batches: classes in order while the union of their targets' rows fits the cap; a batch of one class
  // that does not fit whole is built a window of words at a time
  const uint32_t X = d == 0 ? D : nk;  // population counts per target
  const uint64_t per_t = uint64_t(X + nk) * 8, per_tw = uint64_t(D) * 8;  // bytes per target; per target and word
  std::vector<EffBatch> batches;
  {
    std::vector<uint32_t> stamp(T, 0);
    for (uint32_t ci = 0; ci < cls.size(); ci++) {
      const uint32_t* L = list.data() + l_off[cls[ci].list];
      const uint32_t n = l_len[cls[ci].list];
      for (int attempt = 0; attempt < 2; attempt++) {
        if (batches.empty() || attempt) batches.emplace_back();
        EffBatch& b = batches.back();
        const uint32_t id = uint32_t(batches.size());
        uint32_t fresh = 0;
        for (uint32_t e = 0; e < n; e++) fresh += stamp[L[e]] != id;
        const uint64_t U = b.tl.size() + fresh;
        if (!b.cls.empty() && U * (per_t + per_tw * W) > cap) continue;  // (a new batch takes it)
        if (U * (per_t + per_tw) > cap)
          throw Panic{CYC_ERR_OOM, "target effects: " + std::to_string(U) + " targets apply to one pod; their rows of one word exceed the scratch cap"};
        for (uint32_t e = 0; e < n; e++)
          if (stamp[L[e]] != id) stamp[L[e]] = id, b.tl.push_back(L[e]);
        b.cls.push_back(ci);
        break;
      }
    }
    for (EffBatch& b : batches) {
      std::sort(b.tl.begin(), b.tl.end());
      const uint64_t U = b.tl.size();
      b.WA = uint32_t(std::min<uint64_t>(W, (cap - U * per_t) / (U * per_tw)));
    }
  }

  // ---- the batch buffers, sized for the largest batch
  uint64_t max_a = 0, max_u = 0, max_ct = 0, max_c = 0;
  for (const EffBatch& b : batches) {
    max_a = std::max<uint64_t>(max_a, uint64_t(b.tl.size()) * D * b.WA);
    max_u = std::max<uint64_t>(max_u, b.tl.size());
    uint64_t ct = 0;
    for (uint32_t ci : b.cls) ct += l_len[cls[ci].list];
    max_ct = std::max(max_ct, ct);
    max_c = std::max<uint64_t>(max_c, b.cls.size());
  }
  DevBuf d_a, d_pop, d_sole, d_tl, d_coff, d_ct, d_cn, d_cd;
  d_a.alloc(max_a * 8);
  d_pop.alloc(max_u * X * 8);
  d_sole.alloc(max_u * nk * 8);
  d_tl.alloc(max_u * 4);
  d_coff.alloc((max_c + 1) * 4);
  d_ct.alloc(max_ct * 4);
  d_cn.alloc(max_c * 4);
  d_cd.alloc(std::max<uint64_t>(max_c * nk * 4, 16));
  peak = std::max(peak, fixed + d_a.bytes + d_pop.bytes + d_sole.bytes + d_tl.bytes + d_coff.bytes + d_ct.bytes + d_cn.bytes + d_cd.bytes);
  c->effects.scratch = peak;

  // effects[.][1] and [.][3] hold the applicable VALID cells (of all classes; of one-target classes) until
  // the end; allow1 the ALLOWING cells of one-target classes
  std::vector<int64_t> allow1(size_t(T) * nk, 0);
  std::vector<uint32_t> loc(T, 0), coff, ct, cn;
  std::vector<int32_t> cd;
  std::vector<unsigned long long> pop, sole;
  for (const EffBatch& b : batches) {
    const uint32_t U = uint32_t(b.tl.size());
    for (uint32_t u = 0; u < U; u++) loc[b.tl[u]] = u;
    // the classes of two or more targets, for the sole sweep
    coff.assign(1, 0), ct.clear(), cn.clear(), cd.clear();
    for (uint32_t ci : b.cls) {
      const EffClass& k = cls[ci];
      const uint32_t* L = list.data() + l_off[k.list];
      const uint32_t n = l_len[k.list];
      for (uint32_t kk = 0; kk < nk; kk++) {  // the applicable VALID cells (window-independent)
        const int64_t cells = d == 0 ? (row_desc[size_t(k.row) * nk + kk] >= 0 ? int64_t(P) : 0) : n_valid[kk];
        for (uint32_t e = 0; e < n; e++) {
          int64_t* o = effects + (size_t(L[e]) * nk + kk) * 4;
          o[CYC_EFFECT_DENYING] += cells * k.pods;
          if (n == 1) o[CYC_EFFECT_SOLE_DENYING] += cells * k.pods;
        }
      }
      if (n < 2) continue;
      for (uint32_t e = 0; e < n; e++) ct.push_back(loc[L[e]]);
      coff.push_back(uint32_t(ct.size()));
      cn.push_back(k.pods);
      if (d == 0) cd.insert(cd.end(), row_desc.begin() + size_t(k.row) * nk, row_desc.begin() + size_t(k.row + 1) * nk);
    }
    const uint32_t NC = uint32_t(cn.size());
    HIPCHK(hipMemcpyAsync(d_tl.p, b.tl.data(), size_t(U) * 4, hipMemcpyHostToDevice, st));
    if (NC) {
      HIPCHK(hipMemcpyAsync(d_coff.p, coff.data(), coff.size() * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_ct.p, ct.data(), ct.size() * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_cn.p, cn.data(), cn.size() * 4, hipMemcpyHostToDevice, st));
      if (d == 0) HIPCHK(hipMemcpyAsync(d_cd.p, cd.data(), cd.size() * 4, hipMemcpyHostToDevice, st));
    }
    pop.resize(size_t(U) * X);
    sole.resize(size_t(U) * nk);
    for (uint32_t w0 = 0; w0 < W; w0 += b.WA) {
      const uint32_t WA = std::min(b.WA, W - w0);
      EffRowArgs ra{x, U, w0, WA, d_tl.as<uint32_t>(), d_a.as<uint64_t>()};
      kernel_done(3);  // (uploads, k_eff_valid)
      k_eff_rows<<<grid1(uint64_t(U) * WA * 64, 256), 256, 0, st>>>(ra);
      HIPCHK(hipGetLastError());
      kernel_done(0);
      EffPopArgs pa2{D, W, w0, WA, X, d_a.as<uint64_t>(), V.as<uint64_t>(), d_pop.as<unsigned long long>()};
      if (d == 0) k_eff_pop<false><<<unsigned(uint64_t(U) * X), 256, 0, st>>>(pa2);
      else k_eff_pop<true><<<unsigned(uint64_t(U) * X), 256, 0, st>>>(pa2);
      HIPCHK(hipGetLastError());
      kernel_done(1);
      if (NC) {
        HIPCHK(hipMemsetAsync(d_sole.p, 0, size_t(U) * nk * 8, st));
        EffSoleArgs sa{D, W, w0, WA, nk, NC, d_a.as<uint64_t>(), V.as<uint64_t>(), d_coff.as<uint32_t>(), d_ct.as<uint32_t>(),
                       d_cn.as<uint32_t>(), d_cd.as<int32_t>(), d_sole.as<unsigned long long>()};
        const unsigned nb = grid1(uint64_t(NC) * nk * ((WA + 255) / 256), 1);
        if (d == 0) k_eff_sole<false><<<nb, 256, 0, st>>>(sa);
        else k_eff_sole<true><<<nb, 256, 0, st>>>(sa);
        HIPCHK(hipGetLastError());
        kernel_done(2);
        HIPCHK(hipMemcpyAsync(sole.data(), d_sole.p, sole.size() * 8, hipMemcpyDeviceToHost, st));
      }
      HIPCHK(hipMemcpyAsync(pop.data(), d_pop.p, pop.size() * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      c->effects.launches++;
      for (uint32_t ci : b.cls) {
        const EffClass& k = cls[ci];
        const uint32_t* L = list.data() + l_off[k.list];
        const uint32_t n = l_len[k.list];
        for (uint32_t kk = 0; kk < nk; kk++) {
          const int32_t j = d == 0 ? row_desc[size_t(k.row) * nk + kk] : int32_t(kk);
          if (j < 0) continue;
          for (uint32_t e = 0; e < n; e++) {
            const int64_t v = int64_t(pop[size_t(loc[L[e]]) * X + uint32_t(j)]) * k.pods;
            effects[(size_t(L[e]) * nk + kk) * 4 + CYC_EFFECT_ALLOWING] += v;
            if (n == 1) allow1[size_t(L[e]) * nk + kk] += v;
          }
        }
      }
      if (NC)
        for (uint32_t u = 0; u < U; u++)
          for (uint32_t kk = 0; kk < nk; kk++)
            effects[(size_t(b.tl[u]) * nk + kk) * 4 + CYC_EFFECT_SOLE_ALLOWING] += int64_t(sole[size_t(u) * nk + kk]);
    }
    c->effects.batches++;
  }
  clk.lap("batches");
  if (clk.on)
    fprintf(stderr, "[cyc effects] %lld batches, %lld row builds, %zu classes: k_eff_rows %.2f ms, k_eff_pop %.2f ms, k_eff_sole %.2f ms, other %.2f ms\n",
            (long long)c->effects.batches, (long long)c->effects.launches, cls.size(), k_ms[0], k_ms[1], k_ms[2], k_ms[3]);
  for (size_t i = 0; i < size_t(T) * nk; i++) {
    effects[i * 4 + CYC_EFFECT_DENYING] -= effects[i * 4 + CYC_EFFECT_ALLOWING];
    effects[i * 4 + CYC_EFFECT_SOLE_DENYING] -= allow1[i];
  }
  return (int)CYC_OK;
}
