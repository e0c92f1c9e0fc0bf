/* The part of glib's interface that the reference's priority_queue.c and
 * network_queuing_disciplines.c use, and nothing else.  Written for oracle/ref_qdisc; the
 * functions are in ../shim_glib.c.  First on the include path, so <glib.h> finds this file. */
#ifndef REF_QDISC_SHIM_GLIB_H
#define REF_QDISC_SHIM_GLIB_H

#include <stddef.h>
#include <stdlib.h>

typedef void* gpointer;
typedef const void* gconstpointer;
typedef int gint;
typedef unsigned int guint;
typedef size_t gsize;
typedef gint gboolean;

#ifndef TRUE
#define TRUE 1
#endif
#ifndef FALSE
#define FALSE 0
#endif

typedef gint (*GCompareFunc)(gconstpointer a, gconstpointer b);
typedef gint (*GCompareDataFunc)(gconstpointer a, gconstpointer b, gpointer user_data);
typedef void (*GDestroyNotify)(gpointer data);
typedef guint (*GHashFunc)(gconstpointer key);
typedef gboolean (*GEqualFunc)(gconstpointer a, gconstpointer b);

/* memory: glib aborts when out of memory, so do these */
gpointer shim_alloc(gsize bytes);
gpointer shim_realloc(gpointer mem, gsize bytes);
#define g_new(type, count) ((type*)shim_alloc(sizeof(type) * (gsize)(count)))
#define g_renew(type, mem, count) ((type*)shim_realloc((mem), sizeof(type) * (gsize)(count)))
#define g_free(mem) free(mem)
#define g_slice_new(type) ((type*)shim_alloc(sizeof(type)))
#define g_slice_free(type, mem) free(mem)

/* GHashTable: key -> value, keys compared with the table's own hash and equality functions.
 * Inserting a key equal to a present one keeps the present key and replaces its value. */
typedef struct _GHashTable GHashTable;
GHashTable* g_hash_table_new(GHashFunc hash_func, GEqualFunc key_equal_func);
void g_hash_table_destroy(GHashTable* table);
gboolean g_hash_table_insert(GHashTable* table, gpointer key, gpointer value);
gpointer g_hash_table_lookup(GHashTable* table, gconstpointer key);
gboolean g_hash_table_remove(GHashTable* table, gconstpointer key);
void g_hash_table_remove_all(GHashTable* table);

/* GQueue: only head pops, tail pushes and a linear search */
typedef struct _GList GList;
struct _GList {
    gpointer data;
};
typedef struct _GQueue GQueue;
GQueue* g_queue_new(void);
void g_queue_free(GQueue* queue);
gboolean g_queue_is_empty(GQueue* queue);
gpointer g_queue_pop_head(GQueue* queue);
void g_queue_push_tail(GQueue* queue, gpointer data);
GList* g_queue_find_custom(GQueue* queue, gconstpointer data, GCompareFunc func);

#endif
