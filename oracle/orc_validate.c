/*
 * orc_validate.c — which scene descriptions the oracle accepts.
 *
 * TEST INFRASTRUCTURE ONLY (see rtg_oracle.h).  Not a restatement of the reference, which trusts its
 * parser: these are the index checks of librtg's validate() (rtg_host.cpp), so that a description
 * rtg_scene_create refuses is refused by orc_scene_create too, before anything is built from it.
 */
#include "rtg_oracle.h"

int orc_desc_valid(const rtg_scene_desc* d) {
    if (!d) return 0;
    if (d->num_vertices < 0 || (d->num_vertices && !d->vertices)) return 0;
    if (d->num_objects < 0 || (d->num_objects && !d->objects)) return 0;
    if (d->num_instances < 0 || (d->num_instances && !d->instances)) return 0;
    for (int i = 0; i < d->num_objects; i++) {
        const rtg_object_desc* o = &d->objects[i];
        if (o->material < 1 || o->material > d->num_materials) return 0;
        if (o->num_textures < 0 || o->num_textures > 2) return 0;
        for (int t = 0; t < o->num_textures; t++)
            if (o->textures[t] < 1 || o->textures[t] > d->num_textures) return 0;
    }
    for (int i = 0; i < d->num_instances; i++) {
        const rtg_instance_desc* in = &d->instances[i];
        if (in->base_object < 0 || in->base_object >= d->num_objects) return 0;
        if (in->material < 1 || in->material > d->num_materials) return 0;
    }
    for (int i = 0; i < d->num_textures; i++) {
        const rtg_texture_desc* t = &d->textures[i];
        if (t->kind == RTG_TEX_IMAGE && (t->width < 1 || t->height < 1 || !t->texels)) return 0;
    }
    for (int i = 0; i < d->num_lights; i++)
        if (d->lights[i].type == RTG_LIGHT_ENVIRONMENT &&
            (d->lights[i].texture < 0 || d->lights[i].texture >= d->num_textures)) return 0;
    if (d->background_texture >= d->num_textures) return 0;
    if (d->environment_light >= d->num_lights) return 0;
    return 1;
}
