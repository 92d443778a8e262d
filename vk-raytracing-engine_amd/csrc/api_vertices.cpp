// api_vertices.cpp -- deforming meshes (include/vkrt.h): vertex updates, skins, morphs, their debug reader, and the motion mark that
// snapshots instances and positions.  What the calls refuse is vertex_anim.h's; the kernels are vertex_update.hip, skin.hip, morph.hip.
#include "scene_state.h"
#include "vertex_update.h"

using namespace vkrt;

extern "C" {

int vkrt_scene_update_vertices(vkrt_scene* s, const vkrt_vertex_update* u, void* hip_stream)
{
  CHECK_TRY(check_update_desc(u, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_scene_update_vertices: scene is NULL");
  CHECK_TRY(check_update_range(*u, s->positions.size() / 3, err));
  const bool host = u->memory == VKRT_MEMORY_HOST;
  const size_t n = u->count;
  if(n == 0 || (!u->positions && !u->normals && !u->tangents && !u->texcoords0))
    return VKRT_OK;
  RC_TRY(enter(s));
  hipStream_t stream = (hipStream_t)hip_stream;
  VertexUpdate d;
  d.first = u->first; d.count = u->count;
  d.positions = u->positions; d.normals = u->normals; d.tangents = u->tangents; d.texcoords0 = u->texcoords0;
  if(host)  // the given arrays through the staging buffer, 16-byte elements first, so every part starts aligned for its loads
    HIP_TRY(s->vertexStage.put({{u->tangents, 4 * n, &d.tangents}, {u->texcoords0, 2 * n, &d.texcoords0}, {u->positions, 3 * n, &d.positions},
                                {u->normals, 3 * n, &d.normals}}, stream));
  // Stream-ordered like vkrt_scene_update_nodes: one launch on hip_stream, after whatever still reads the old vertices and before the
  // refit and the next trace (whose internal lane streams fork from and join to the caller's stream).
  HIP_TRY(launch_vertex_update(const_cast<float*>(s->dev.positions), const_cast<float4*>(s->dev.vertexPN), d, stream));
  if(host)
  {
    HIP_TRY(hipStreamSynchronize(stream));  // the caller's arrays and the staging buffer are free again
    if(u->positions)
      std::copy(u->positions, u->positions + 3 * n, s->positions.begin() + 3 * (size_t)u->first);
  }
  if(u->positions)
    positionsMoved(s, host);
  return VKRT_OK;
}

int vkrt_scene_add_skin(vkrt_scene* s, const vkrt_skin_desc* k, void* hip_stream, uint32_t* out_skin)
{
  const char* who = "vkrt_scene_add_skin";
  CHECK_TRY(check_skin_desc(k, err));
  if(!out_skin)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: out_skin is NULL", who);
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_skin_range(*k, s->positions.size() / 3, rangesOf(s->skins), rangesOf(s->morphs), err));
  RC_TRY(enter(s));
  const size_t n = k->count;
  vkrt_scene::Skin skin;
  skin.jointCount = k->joint_count;
  HIP_TRY(skin.mem.alloc(skin_bytes(k->count)));
  skin_carve(skin.mem.get(), k->first, k->count, skin.arrays);
  HIP_TRY(hipMemcpy(skin.arrays.joints, k->joints, n * 4 * sizeof(uint16_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(skin.arrays.weights, k->weights, n * 4 * sizeof(float), hipMemcpyHostToDevice));
  // stream-ordered like the update calls: the bind pose is what the updates enqueued before this call on hip_stream left
  HIP_TRY(launch_pose_capture(s->dev.positions, s->dev.vertexPN, k->first, k->count, skin.arrays.bind, (hipStream_t)hip_stream));
  *out_skin = (uint32_t)s->skins.size();
  s->skins.push_back(std::move(skin));
  return VKRT_OK;
}

int vkrt_scene_skin_vertices(vkrt_scene* s, uint32_t skin, const float* joint_matrices, uint32_t memory, void* hip_stream)
{
  const char* who = "vkrt_scene_skin_vertices";
  CHECK_TRY(check_memory(who, memory, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_skin_index(skin, s->skins.size(), err));
  const vkrt_scene::Skin& k = s->skins[skin];
  CHECK_TRY(check_joint_matrices(joint_matrices, memory, k.jointCount, err));
  const bool host = memory == VKRT_MEMORY_HOST;
  RC_TRY(enter(s));
  hipStream_t stream = (hipStream_t)hip_stream;
  const float* palette = joint_matrices;
  if(host)
    HIP_TRY(s->vertexStage.put({{joint_matrices, (size_t)k.jointCount * 16, &palette}}, stream));
  HIP_TRY(launch_skin(const_cast<float*>(s->dev.positions), const_cast<float4*>(s->dev.vertexPN), k.arrays, (const float4*)palette, stream));
  if(host)
    HIP_TRY(hipStreamSynchronize(stream));  // the caller's matrices and the staging buffer are free again
  positionsMoved(s);  // (host matrices too: the posed positions exist on the device only)
  return VKRT_OK;
}

int vkrt_scene_add_morph(vkrt_scene* s, const vkrt_morph_desc* m, void* hip_stream, uint32_t* out_morph)
{
  const char* who = "vkrt_scene_add_morph";
  CHECK_TRY(check_morph_desc(m, err));
  if(!out_morph)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: out_morph is NULL", who);
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  int inSkin = -1;
  CHECK_TRY(check_morph_range(*m, s->positions.size() / 3, rangesOf(s->skins), rangesOf(s->morphs), inSkin, err));
  RC_TRY(enter(s));
  const size_t n = m->count, floats = (size_t)m->target_count * n * 3;
  const float* const deltas[3] = {m->position_deltas, m->normal_deltas, m->tangent_deltas};
  vkrt_scene::Morph morph;
  morph.skin = inSkin;
  const bool has[3] = {deltas[0] != nullptr, deltas[1] != nullptr, deltas[2] != nullptr};
  if(morph.mem.alloc(morph_bytes(m->count, m->target_count, has[0], has[1], has[2])) != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(VKRT_ERR_OUT_OF_MEMORY, "%s: no device memory for %u targets of %u vertices", who, m->target_count, m->count);
  }
  MorphArrays& a = morph.arrays;
  morph_carve(morph.mem.get(), m->first, m->count, m->target_count, has[0], has[1], has[2], a);
  float* const dst[3] = {a.dPos, a.dNrm, a.dTan};
  for(int i = 0; i < 3; i++)
    if(deltas[i])
      HIP_TRY(hipMemcpy(dst[i], deltas[i], floats * sizeof(float), hipMemcpyHostToDevice));
  // stream-ordered like the update calls: the base is what the calls enqueued before this one on hip_stream left
  hipStream_t stream = (hipStream_t)hip_stream;
  if(inSkin < 0)
    HIP_TRY(launch_pose_capture(s->dev.positions, s->dev.vertexPN, a.first, a.count, a.base, stream));
  else
  {
    const SkinArrays& k = s->skins[inSkin].arrays;
    const Pose bind = k.bind.at(m->first - k.first);
    HIP_TRY(hipMemcpyAsync(a.base.pn, bind.pn, n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(a.base.nyz, bind.nyz, n * sizeof(float2), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(a.base.tan, bind.tan, n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
  }
  *out_morph = (uint32_t)s->morphs.size();
  s->morphs.push_back(std::move(morph));
  return VKRT_OK;
}

int vkrt_scene_morph_vertices(vkrt_scene* s, uint32_t morph, const float* weights, uint32_t memory, void* hip_stream)
{
  const char* who = "vkrt_scene_morph_vertices";
  CHECK_TRY(check_memory(who, memory, err));
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_morph_index(morph, s->morphs.size(), err));
  const vkrt_scene::Morph& m = s->morphs[morph];
  CHECK_TRY(check_morph_weights(weights, memory, m.arrays.targetCount, err));
  const bool host = memory == VKRT_MEMORY_HOST;
  RC_TRY(enter(s));
  hipStream_t stream = (hipStream_t)hip_stream;
  const float* w = weights;
  if(host)
    HIP_TRY(s->vertexStage.put({{weights, m.arrays.targetCount, &w}}, stream));
  if(m.skin >= 0)
  {  // morph, then skin: the skin's next pose reads the morphed bind pose; the live arrays and the tree are as they were
    const SkinArrays& k = s->skins[m.skin].arrays;
    HIP_TRY(launch_morph_bind(k.bind.at(m.arrays.first - k.first), m.arrays, w, stream));
  }
  else
    HIP_TRY(launch_morph_live(const_cast<float*>(s->dev.positions), const_cast<float4*>(s->dev.vertexPN), m.arrays, w, stream));
  if(host)
    HIP_TRY(hipStreamSynchronize(stream));  // the caller's weights and the staging buffer are free again
  if(m.skin < 0)
    positionsMoved(s);  // (host weights too: the morphed positions exist on the device only; inside a skin no live vertex moved)
  return VKRT_OK;
}

int vkrt_debug_read_vertices(vkrt_scene* s, uint32_t first, uint32_t count, float* positions, float* normals, float* tangents, float* texcoords0)
{
  const char* who = "vkrt_debug_read_vertices";
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: scene is NULL", who);
  CHECK_TRY(check_vertex_range(who, first, count, s->positions.size() / 3, err));
  if(!positions && !normals && !tangents && !texcoords0)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "%s: positions, normals, tangents and texcoords0 are all NULL", who);
  RC_TRY(enter(s));
  const size_t n = count;
  HIP_TRY(readBack(positions, s->dev.positions + 3 * (size_t)first, positions ? n * 3 * sizeof(float) : 0));
  if(n && (normals || tangents || texcoords0))
  {  // quad 0 = position.xyz, normal.x; quad 1 = normal.yz, uv; quad 2 = tangent
    std::vector<float> rec(n * 4 * VKRT_VERTEX_QUADS);
    HIP_TRY(hipMemcpy(rec.data(), s->dev.vertexPN + VKRT_VERTEX_QUADS * (size_t)first, rec.size() * sizeof(float), hipMemcpyDeviceToHost));
    for(size_t i = 0; i < n; i++)
    {
      const float* r = &rec[i * 4 * VKRT_VERTEX_QUADS];
      if(normals)
        normals[3 * i] = r[3], normals[3 * i + 1] = r[4], normals[3 * i + 2] = r[5];
      if(texcoords0)
        texcoords0[2 * i] = r[6], texcoords0[2 * i + 1] = r[7];
      if(tangents)
        std::copy(r + 8, r + 12, tangents + 4 * i);
    }
  }
  return VKRT_OK;
}

int vkrt_scene_motion_mark(vkrt_scene* s, void* hip_stream)
{
  if(!s)
    return fail(VKRT_ERR_INVALID_ARGUMENT, "vkrt_scene_motion_mark: scene is NULL");
  RC_TRY(enter(s));
  const size_t instBytes = s->nodes.size() * sizeof(DevInstance), posBytes = s->positions.size() * sizeof(float);
  if(!s->motion.get())
  {  // first mark: the one place a mark allocates (and, through hipMalloc, may synchronise)
    const hipError_t e = s->motion.alloc(s->motionPositionsAt() + std::max<size_t>(posBytes, 16));
    if(e != hipSuccess)
      return fail(e == hipErrorOutOfMemory ? VKRT_ERR_OUT_OF_MEMORY : VKRT_ERR_HIP, "vkrt_scene_motion_mark: hipMalloc: %s", hipGetErrorString(e));
  }
  // Stream-ordered like the two update calls: the copies read what the updates enqueued before them on hip_stream wrote, and are read
  // by what comes after (vkrt_hit_motion).  Nothing here depends on the tree, so a build or a refit leaves the snapshot alone.
  hipStream_t stream = (hipStream_t)hip_stream;
  if(instBytes)
    HIP_TRY(hipMemcpyAsync(const_cast<DevInstance*>(s->prevInstances()), s->dev.instances, instBytes, hipMemcpyDeviceToDevice, stream));
  if(posBytes)
    HIP_TRY(hipMemcpyAsync(const_cast<float*>(s->prevPositions()), s->dev.positions, posBytes, hipMemcpyDeviceToDevice, stream));
  return VKRT_OK;
}

}  // extern "C"
